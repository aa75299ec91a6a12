"""``rtts_align_stats`` and ``rtts_align_mas`` (csrc/align.hip) on the GPU against their float64 restatement (tests/align_ref.py).

Exact cases use matrices whose sums are exact in any order (multiples of 2^-10, constants): every integer output, every exact
column of the table and the path mass must equal the restatement bit for bit.  The float64 cases check entropy, guided weight and
Q to rtol = atol = 1e-10: both sides work in f64 from identical f32 inputs and differ only in the order of the sums and in the
last place of log / exp, about (T_k + T_q) 2^-53 = 7e-13 relative.  Durations are compared exactly wherever the restatement's own
decision margin is at least 1e-6, a thousand times the accumulated f64 error of Q at these sizes; the test asserts the margin
first."""
import numpy as np
import pytest
import torch

import align_ref as ref

pytestmark = pytest.mark.gpu

SIGMA = 0.2
EXACT_COLS = [0, 1, 2, 3, 6, 7]        # on matrices whose sums are exact in any order
COUNT_COLS = [0, 1, 6, 7]
T_EDGES = (1, 15, 16, 17, 63, 64, 65)
K_EDGES = (1, 63, 64, 65, 127, 128, 129)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _i32(values, gpu):
    return torch.tensor([int(v) for v in values], dtype=torch.int32).to(gpu)


def _run(mats, nf, nk, gpu, floor=1e-30):
    """Both entries on (L, B, Tq, Tk) numpy matrices -> a dict of numpy outputs."""
    from reformer_tts_amd import ops
    dev = mats if torch.is_tensor(mats) or isinstance(mats, list) else torch.from_numpy(mats).to(gpu)
    f, k = _i32(nf, gpu), _i32(nk, gpu)
    argmax, dur_a, table = ops.alignment_stats(dev, f, k, SIGMA)
    dur, path, scores = ops.alignment_mas(dev, f, k, floor)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in dict(argmax=argmax, dur_argmax=dur_a, table=table, durations=dur, path=path, scores=scores).items()}


def _want(mats, nf, nk, floor=1e-30):
    argmax, dur_a, table = ref.stats_batch_ref(mats, nf, nk, SIGMA)
    dur, path, scores, margins = ref.mas_batch_ref(mats, nf, nk, floor)
    return dict(argmax=argmax, dur_argmax=dur_a, table=table, durations=dur, path=path, scores=scores, margins=margins)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check_integers(got, want):
    for name in ("argmax", "dur_argmax", "durations", "path"):
        assert got[name].dtype == np.int32 and _same(got[name], want[name]), name


def _check_close(got, want):
    """The counts exactly, the f64 sums to 1e-10; NaN rows must be NaN on both sides."""
    assert _same(got["table"][..., COUNT_COLS], want["table"][..., COUNT_COLS])
    for name in ("table", "scores"):
        assert _same(np.isnan(got[name]), np.isnan(want[name])), name
        np.testing.assert_allclose(got[name], want[name], rtol=1e-10, atol=1e-10, equal_nan=True, err_msg=name)


def _lengths(tq, tk):
    """(T, K) pairs over the edges that fit, with T = K (a forced diagonal) and T = K + 1 for every K edge."""
    ts = [t for t in T_EDGES + (tq,) if t <= tq]
    ks = [k for k in K_EDGES + (tk,) if k <= tk]
    pairs = [(t, k) for t in ts for k in ks]
    pairs += [(k, k) for k in ks if k <= tq] + [(k + 1, k) for k in ks if k + 1 <= tq]
    return sorted(set(pairs))


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("tq,tk", [(64, 128), (192, 256), (320, 128)])
def test_exact_on_dyadic_and_constant_matrices(gpu, tq, tk):
    pairs = _lengths(tq, tk)
    nf, nk = [p[0] for p in pairs], [p[1] for p in pairs]
    mats = np.stack([np.stack([ref.dyadic(tq, tk, t, k, 1000 * tq + 7 * i) for i, (t, k) in enumerate(pairs)]),
                     np.stack([ref.constant(tq, tk)] * len(pairs))])
    got, want = _run(mats, nf, nk, gpu), _want(mats, nf, nk)
    scorable = ~np.isnan(want["margins"][0])
    assert scorable.sum() >= 8 and (~scorable).sum() >= 4                      # T < K slots are part of the batch
    assert np.nanmin(want["margins"][0]) >= 1e-6                                  # the dyadic ridge leaves no near-tie
    _check_integers(got, want)
    assert _same(got["table"][..., EXACT_COLS], want["table"][..., EXACT_COLS])
    assert _same(got["scores"][..., 1], want["scores"][..., 1])
    assert _same(got["scores"][1, :, 0], want["scores"][1, :, 0])                # Q on the constant matrices
    _check_close(got, want)
    ok = np.array(nf) >= np.array(nk)
    assert np.all(got["durations"][:, ok].sum(-1) == np.array(nf)[ok])
    assert all(got["durations"][m, b, :nk[b]].min() >= 1 for m in range(2) for b in np.flatnonzero(ok))
    assert np.isnan(got["scores"][:, -1]).all() and not np.isnan(got["table"][:, -1]).any()      # T < K: unscorable for the search only


# ------------------------------------------------------------------ against float64
def _noisy_batch(tq, tk, shapes, seed):
    diag = np.stack([ref.noisy_diagonal(tq, tk, t, k, 40.0 + 10 * i, 1.0, seed + i) for i, (t, k) in enumerate(shapes)])
    noise = np.stack([ref.pure_noise(tq, tk, seed + 100 + i) for i in range(len(shapes))])
    return np.stack([diag, noise])


F64_CASES = [
    (320, 256, [(320, 256), (150, 129), (65, 64), (17, 1), (100, 100)], 11),
    (320, 128, [(320, 128), (257, 127), (300, 65), (129, 128), (16, 15)], 23),
    (192, 2048, [(192, 130), (150, 100), (129, 129), (64, 1), (192, 65)], 37),       # two keys per lane, back-pointers in LDS
]


@pytest.mark.parametrize("tq,tk,shapes,seed", F64_CASES)
def test_against_float64(gpu, tq, tk, shapes, seed):
    mats = _noisy_batch(tq, tk, shapes, seed)
    nf, nk = [s[0] for s in shapes], [s[1] for s in shapes]
    got, want = _run(mats, nf, nk, gpu), _want(mats, nf, nk)
    print(f"\n[align f64 {tq}x{tk}] margins {want['margins'].tolist()}")
    print(f"  entropy err {np.abs(got['table'][..., 4] - want['table'][..., 4]).max():.2e}  guided err "
          f"{np.abs(got['table'][..., 5] - want['table'][..., 5]).max():.2e}  Q err {np.abs(got['scores'][..., 0] - want['scores'][..., 0]).max():.2e}")
    assert np.min(want["margins"]) >= 1e-6
    _check_close(got, want)
    _check_integers(got, want)


@pytest.mark.parametrize("tq,tk,t,k,seed,in_lds", [(1600, 2048, 1600, 1500, 5, False), (4096, 512, 4000, 500, 9, False),
                                                   (4096, 256, 3900, 250, 13, True)])
def test_larger_cases(gpu, tq, tk, t, k, seed, in_lds):
    """More than one key per lane; a bit table that cannot live in LDS (both read it from the workspace); and the largest one that
    can (more than 64 KB of LDS)."""
    from reformer_tts_amd import ops
    assert (ops._lib.load().rtts_align_mas_workspace(1, 1, tq, tk) >= tq * tk // 8) == (not in_lds)
    mats = ref.noisy_diagonal(tq, tk, t, k, 200.0, 1.0, seed)[None, None]
    got, want = _run(mats, [t], [k], gpu), _want(mats, [t], [k])
    print(f"\n[align large {tq}x{tk}] margin {want['margins'].tolist()}")
    assert np.min(want["margins"]) >= 1e-6
    _check_close(got, want)
    _check_integers(got, want)
    assert got["durations"][0, 0].sum() == t and got["durations"][0, 0, :k].min() >= 1 and not got["durations"][0, 0, k:].any()


# ------------------------------------------------------------------ other behaviour
@pytest.fixture(scope="module")
def batch():
    tq, tk = 320, 256
    shapes = [(320, 256), (150, 129), (65, 64), (17, 1), (100, 100), (130, 200)]        # the last: fewer frames than keys
    mats = _noisy_batch(tq, tk, shapes, 51)
    return mats, [s[0] for s in shapes], [s[1] for s in shapes]


def test_alone_again_and_captured(gpu, batch):
    from reformer_tts_amd import ops
    mats, nf, nk = batch
    whole = _run(mats, nf, nk, gpu)
    again = _run(mats, nf, nk, gpu)
    for name in whole:
        assert _same(whole[name], again[name]), name
    for b in range(len(nf)):
        alone = _run(np.ascontiguousarray(mats[:, b:b + 1]), nf[b:b + 1], nk[b:b + 1], gpu)
        for name in whole:
            assert _same(alone[name][:, 0], whole[name][:, b]), (name, b)
    dev, f, k = torch.from_numpy(mats).to(gpu), _i32(nf, gpu), _i32(nk, gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.alignment_stats(dev, f, k, SIGMA)
        ops.alignment_mas(dev, f, k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = (*ops.alignment_stats(dev, f, k, SIGMA), *ops.alignment_mas(dev, f, k))
    for o in outs:
        o.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for name, o in zip(("argmax", "dur_argmax", "table", "durations", "path", "scores"), outs):
        assert _same(o.cpu().numpy(), whole[name]), name
    # the lengths are read on the device: the same graph scores other lengths
    f.copy_(_i32([n - 1 for n in nf], gpu))
    graph.replay()
    torch.cuda.synchronize()
    other = _run(mats, [n - 1 for n in nf], nk, gpu)
    for name, o in zip(("argmax", "dur_argmax", "table", "durations", "path", "scores"), outs):
        assert _same(o.cpu().numpy(), other[name]), name


def test_stacked_listed_and_strided_operands_agree(gpu, batch):
    mats, nf, nk = batch
    whole = _run(mats, nf, nk, gpu)
    dev = torch.from_numpy(mats).to(gpu)
    separate = [dev[0].clone(), dev[1].clone()]                                 # two allocations: stacked by the wrapper
    in_place = [dev[0], dev[1]]                                                 # already one buffer, read where they lie
    wide = torch.full((2, len(nf), 320, 256 + 20), float("nan"), device=gpu)    # ld > T_k, NaN between the rows
    wide[..., :256] = dev
    for operand in (separate, in_place, wide[..., :256], [wide[0, :, :, :256], wide[1, :, :, :256]]):
        got = _run(operand, nf, nk, gpu)
        for name in whole:
            assert _same(got[name], whole[name]), name


def test_refusals_on_the_device(gpu):
    from reformer_tts_amd import ops
    f = _i32([4, 4], gpu)
    with pytest.raises(ValueError, match="T_k"):
        ops.alignment_stats(torch.zeros(1, 2, 8, 2052, device=gpu), f, f)
    with pytest.raises(ValueError, match="T_q"):
        ops.alignment_mas(torch.zeros(1, 2, 4100, 8, device=gpu), f, f)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.alignment_stats(torch.zeros(1, 2, 8, 6, device=gpu), f, f)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.alignment_mas(torch.zeros(1, 2, 8, 12, device=gpu).view(-1)[1:1 + 64].view(1, 2, 4, 8), f, f)
    with pytest.raises(ValueError, match="n_frames"):
        ops.alignment_stats(torch.zeros(1, 2, 8, 8, device=gpu), _i32([4, 4, 4], gpu), f)
    with pytest.raises(ops._lib.RttsError, match="n_keys must be a CUDA torch.int32"):
        ops.alignment_mas(torch.zeros(1, 2, 8, 8, device=gpu), f, f.long())


def test_unscorable_slots(gpu, batch):
    """n_frames 0 or past T_q, n_keys past T_k, T < K (the search only), a NaN or inf inside the region: the slot and the totals
    row are NaN / 0 / -1, every other slot keeps its bits.  A NaN outside every region changes nothing."""
    mats, nf, nk = batch
    clean = _run(mats, nf, nk, gpu)
    dirty = mats.copy()
    dirty[:, 0, 320 - 1, 255] = np.nan          # slot 0 is (320, 256): the last cell of its region
    dirty[1, 2, 10, 20] = np.inf                # slot 2, second matrix only
    dirty[:, 1, 150:, :] = np.nan               # outside slot 1's region (150, 129)
    dirty[:, 1, :, 129:] = np.nan
    f2, k2 = list(nf), list(nk)
    f2[3] = 0                                   # slot 3: no frame
    f2[4], k2[4] = 60, 100                      # slot 4: fewer frames than keys
    got = _run(dirty, f2, k2, gpu)
    want = _want(dirty, f2, k2)
    _check_integers(got, want)
    _check_close(got, want)
    assert _same(got["scores"][..., 1], want["scores"][..., 1])
    for name in clean:                          # slots 1 and 5 everywhere, slot 2 in the first matrix: the clean bits
        for b in (1, 5):
            assert _same(got[name][:, b], clean[name][:, b]), (name, b)
        assert _same(got[name][0, 2], clean[name][0, 2]), name
    for m, b in ((0, 0), (1, 0), (1, 2), (0, 3), (1, 3)):
        assert np.isnan(got["table"][m, b]).all() and np.isnan(got["scores"][m, b]).all()
        assert (got["argmax"][m, b] == -1).all() and (got["path"][m, b] == -1).all()
        assert not got["dur_argmax"][m, b].any() and not got["durations"][m, b].any()
    assert np.isnan(got["scores"][:, 4]).all() and not got["durations"][:, 4].any() and not np.isnan(got["table"][:, 4]).any()
    assert np.isnan(got["table"][:, -1]).all() and np.isnan(got["scores"][:, -1]).all()
    for bad_f, bad_k in (([321] + nf[1:], nk), (nf, [257] + nk[1:]), ([-1] + nf[1:], nk), (nf, [0] + nk[1:])):
        got = _run(mats, bad_f, bad_k, gpu)
        assert np.isnan(got["table"][:, 0]).all() and np.isnan(got["scores"][:, 0]).all() and (got["argmax"][:, 0] == -1).all()
        for name in clean:
            assert _same(got[name][:, 1:len(nf)], clean[name][:, 1:len(nf)]), name


def test_scores_durations_and_the_most_focused_layer(gpu):
    from reformer_tts_amd import evaluation
    tq, tk, shapes = 128, 64, [(128, 64), (100, 50), (1, 1), (40, 40)]
    layers = [np.stack([ref.noisy_diagonal(tq, tk, t, k, sharp, 0.5, 70 + i) for i, (t, k) in enumerate(shapes)]) for sharp in (5.0, 400.0, 30.0)]
    mats = np.stack(layers)
    nf, nk = [s[0] for s in shapes], [s[1] for s in shapes]
    want = _want(mats, nf, nk)
    dev = [torch.from_numpy(m).to(gpu) for m in layers]
    scores = evaluation.alignment_scores(dev, torch.tensor(nf).to(gpu), torch.tensor(nk).to(gpu), SIGMA)       # int64 lengths are converted
    durs = evaluation.alignment_durations(dev, _i32(nf, gpu), _i32(nk, gpu))
    layer = evaluation.most_focused_layer(scores)
    assert layer.is_cuda and layer.dtype == torch.int64 and int(layer) == 1
    tab = want["table"][:, :-1]
    t, k = tab[..., 0], tab[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        figures = dict(focus=tab[..., 3] / t, entropy=np.where(k == 1, 0.0, tab[..., 4] / t / np.log(k)), guided=tab[..., 5] / t,
                       monotonic=tab[..., 6] / (t - 1), coverage=tab[..., 7] / k, mass=tab[..., 2] / t)
    for name, w in figures.items():
        g = scores[name]
        assert g.shape == (3, 4) and g.dtype == torch.float64 and g.is_cuda
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=1e-10, atol=1e-10, equal_nan=True, err_msg=name)
    assert np.isnan(figures["monotonic"][:, 2]).all() and np.all(figures["entropy"][:, 2] == 0)
    assert _same(scores["argmax"].cpu().numpy(), want["argmax"]) and _same(scores["durations"].cpu().numpy(), want["dur_argmax"])
    assert np.min(want["margins"][:, [0, 1]]) >= 1e-6
    assert _same(durs["durations"].cpu().numpy(), want["durations"]) and _same(durs["path"].cpu().numpy(), want["path"])
    np.testing.assert_allclose(durs["log_prob"].cpu().numpy(), want["scores"][:, :-1, 0] / np.array(nf), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(durs["path_mass"].cpu().numpy(), want["scores"][:, :-1, 1] / np.array(nf), rtol=1e-10, atol=1e-10)
