"""``rtts_sw_inv1x1_factor`` on the GPU: W^-1, sign det W and log|det W| of the invertible 1x1 convolutions against float64 LAPACK
within the derived bounds of tests/sw_lu_ref.py (sign exact), batches bit for bit equal to the matrices factored alone, a
singular matrix between two regular ones, guard words behind every output, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import sw_lu_ref as lu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _s():
    return torch.cuda.current_stream().cuda_stream


GUARD = 64          # words behind every output that must keep their pattern
PATTERN = 12345.0


def _factor_raw(mats, gpu):
    """One launch through the C ABI, outputs pre-filled with NaN, ``GUARD`` words of ``PATTERN`` behind each ->
    ([inverse (n, n) fp32 on the host], slogdet (count, 2) float64 on the host); asserts the guards."""
    from reformer_tts_amd import _lib
    cnt = len(mats)
    wd = [torch.from_numpy(np.ascontiguousarray(m)).to(gpu) for m in mats]
    outs = []
    for m in mats:
        n = m.shape[0]
        o = torch.full((n * n + GUARD,), float("nan"), device=gpu)
        o[n * n:] = PATTERN
        outs.append(o)
    sd = torch.full((2 * cnt + GUARD,), float("nan"), dtype=torch.float64, device=gpu)
    sd[2 * cnt:] = PATTERN
    _lib.call("rtts_sw_inv1x1_factor", (C.c_void_p * cnt)(*[w.data_ptr() for w in wd]), (C.c_int * cnt)(*[m.shape[0] for m in mats]), cnt,
              (C.c_void_p * cnt)(*[o.data_ptr() for o in outs]), sd.data_ptr(), _s())
    torch.cuda.synchronize()
    inv = []
    for m, o in zip(mats, outs):
        n = m.shape[0]
        o = o.cpu()
        assert torch.all(o[n * n:] == PATTERN), "words behind winv were written"
        inv.append(o[:n * n].view(n, n).numpy())
    sd = sd.cpu()
    assert torch.all(sd[2 * cnt:] == PATTERN), "words behind slogdet were written"
    return inv, sd[:2 * cnt].view(cnt, 2).numpy()


@pytest.fixture(scope="module")
def alone(gpu):
    """(kind, n) -> (matrix, inverse, (sign, log|det|)) factored ALONE, once; never modified."""
    cache = {}

    def get(kind, n):
        if (kind, n) not in cache:
            w = lu.matrix(kind, n)
            inv, sd = _factor_raw([w], gpu)
            cache[(kind, n)] = (w, inv[0], sd[0])
        return cache[(kind, n)]
    return get


@pytest.mark.parametrize("kind,n", lu.CASES)
def test_factor_vs_float64(alone, kind, n):
    """Every size and kind, one matrix per launch: sign exact, log|det| and every element of the inverse within the bounds
    (kappa computed here from the reference); the outputs are fully overwritten (no NaN of the pre-fill is left)."""
    w, inv, (sign, logabs) = alone(kind, n)
    assert np.isfinite(inv).all() and np.isfinite(logabs)
    same_sign, r_ld, r_inv, rsign = lu.ratios(inv, sign, logabs, w)
    print(kind, n, "sign", sign, "log-det ratio", r_ld, "inverse ratio", r_inv)
    assert same_sign, (sign, rsign)
    assert r_ld <= 1 and r_inv <= 1, (r_ld, r_inv)
    if kind == "pivoting":
        assert sign == -1


def test_default_model_batch_is_bitwise_the_matrices_alone(gpu, alone):
    """The twelve sizes of the default model in ONE launch (kinds mixed): every output bit for bit that of the matrix alone."""
    kinds = ["orthonormal", "gaussian", "kappa1e5", "pivoting"]
    cases = [(kinds[i % 4], n) for i, n in enumerate(lu.DEFAULT_MODEL_SIZES)]
    mats = [lu.matrix(k, n) for k, n in cases]
    inv, sd = _factor_raw(mats, gpu)
    for i, (k, n) in enumerate(cases):
        _, inv1, sd1 = alone(k, n)
        assert np.array_equal(inv[i].view(np.uint32), inv1.view(np.uint32)), (k, n)
        assert np.array_equal(sd[i].view(np.uint64), sd1.view(np.uint64)), (k, n)
        same_sign, r_ld, r_inv, _ = lu.ratios(inv[i], sd[i][0], sd[i][1], mats[i])
        assert same_sign and r_ld <= 1 and r_inv <= 1, (k, n, r_ld, r_inv)


def test_sixteen_work_and_seventeen_are_refused(gpu, alone):
    from reformer_tts_amd import _lib
    sizes = [1, 2, 6, 8, 48, 112, 128, 8] * 2
    mats = [lu.matrix("gaussian", n) for n in sizes]
    inv, sd = _factor_raw(mats, gpu)
    for i, n in enumerate(sizes):
        _, inv1, sd1 = alone("gaussian", n)
        assert np.array_equal(inv[i].view(np.uint32), inv1.view(np.uint32)) and np.array_equal(sd[i].view(np.uint64), sd1.view(np.uint64)), (i, n)
    with pytest.raises(_lib.RttsError, match=r"count must be 1\.\.16 \(got 17\)"):
        _factor_raw(mats + [mats[0]], gpu)


def test_wrapper_batches_of_more_than_sixteen(gpu, alone):
    """``ops.sw_inv1x1_factor`` (what ``SqueezeWave._fold`` calls) takes any number of matrices: 17 = two launches."""
    from reformer_tts_amd import _lib, ops
    sizes = [8, 48, 6] * 5 + [2, 1]
    ws = [torch.from_numpy(lu.matrix("orthonormal", n)).to(gpu) for n in sizes]
    inv, sd = ops.sw_inv1x1_factor(ws)
    assert sd.shape == (17, 2) and sd.dtype == torch.float64 and sd.device == gpu
    sd = sd.cpu().numpy()
    for i, n in enumerate(sizes):
        _, inv1, sd1 = alone("orthonormal", n)
        assert inv[i].shape == (n, n) and inv[i].dtype == torch.float32
        assert np.array_equal(inv[i].cpu().numpy().view(np.uint32), inv1.view(np.uint32)) and np.array_equal(sd[i].view(np.uint64), sd1.view(np.uint64))
    with pytest.raises(_lib.RttsError, match="GPU only"):
        ops.sw_inv1x1_factor([ws[0].cpu()])


@pytest.mark.parametrize("n", [6, 128])
def test_singular_matrix_between_two_regular_ones(gpu, alone, n):
    """One zero column: sign 0, -inf, an all-NaN inverse; both neighbours bit for bit what they are alone."""
    a, b = lu.matrix("orthonormal", 48), lu.matrix("gaussian", 112)
    inv, sd = _factor_raw([a, lu.singular(n), b], gpu)
    assert sd[1][0] == 0 and sd[1][1] == -np.inf and np.isnan(inv[1]).all()
    for i, k, m in ((0, "orthonormal", 48), (2, "gaussian", 112)):
        _, inv1, sd1 = alone(k, m)
        assert np.array_equal(inv[i].view(np.uint32), inv1.view(np.uint32)) and np.array_equal(sd[i].view(np.uint64), sd1.view(np.uint64))


def test_matrix_with_a_tied_first_column(gpu):
    """Rows 0 and 2 hold the same |a| in the first column: whichever the kernel takes, sign and log|det| are the restatement's and
    the inverse is LAPACK's to fp32.  (This does NOT tell the tie rules apart: on this matrix both give the same values.)"""
    w = np.array([[2, 1, 0], [1, 3, 1], [-2, 0, 4]], dtype=np.float32)
    inv, sd = _factor_raw([w], gpu)
    _, sign, logabs = lu.factor(w)
    assert sd[0][0] == sign and abs(sd[0][1] - logabs) <= 1e-14
    assert np.abs(inv[0].astype(np.float64) - np.linalg.inv(w.astype(np.float64))).max() <= 2.0 ** -23


def test_refusals_launch_nothing(gpu):
    from reformer_tts_amd import _lib
    w = torch.from_numpy(lu.matrix("gaussian", 8)).to(gpu)
    out = torch.full((64,), float("nan"), device=gpu)
    sd = torch.full((4,), float("nan"), dtype=torch.float64, device=gpu)
    ptrs = lambda *p: (C.c_void_p * len(p))(*p)          # noqa: E731
    ints = lambda *v: (C.c_int * len(v))(*v)             # noqa: E731
    one = (ptrs(w.data_ptr()), ints(8), 1, ptrs(out.data_ptr()), sd.data_ptr())
    with pytest.raises(_lib.RttsError, match=r"n\[0\] must be 1\.\.128 \(got 0\)"):
        _lib.call("rtts_sw_inv1x1_factor", one[0], ints(0), 1, one[3], one[4], _s())
    with pytest.raises(_lib.RttsError, match=r"n\[1\] must be 1\.\.128 \(got 129\)"):
        _lib.call("rtts_sw_inv1x1_factor", ptrs(w.data_ptr(), w.data_ptr()), ints(8, 129), 2, ptrs(out.data_ptr(), out.data_ptr()), one[4], _s())
    with pytest.raises(_lib.RttsError, match=r"count must be 1\.\.16 \(got 0\)"):
        _lib.call("rtts_sw_inv1x1_factor", one[0], one[1], 0, one[3], one[4], _s())
    with pytest.raises(_lib.RttsError, match=r"w\[0\] is null"):
        _lib.call("rtts_sw_inv1x1_factor", ptrs(None), one[1], 1, one[3], one[4], _s())
    with pytest.raises(_lib.RttsError, match=r"winv\[0\] is null"):
        _lib.call("rtts_sw_inv1x1_factor", one[0], one[1], 1, ptrs(None), one[4], _s())
    with pytest.raises(_lib.RttsError, match="slogdet is null"):
        _lib.call("rtts_sw_inv1x1_factor", one[0], one[1], 1, one[3], None, _s())
    with pytest.raises(_lib.RttsError, match="w is null"):
        _lib.call("rtts_sw_inv1x1_factor", None, one[1], 1, one[3], one[4], _s())
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(sd).all()
