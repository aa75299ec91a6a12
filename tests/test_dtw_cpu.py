"""The float64 restatement of ``rtts_dtw_align`` (tests/dtw_ref.py) against brute-force enumeration of every monotone path, the
cepstral basis of ``evaluation.cepstral_basis``, the three new symbols of the C ABI and the host-side argument checks of
``ops.dtw_align``.  No GPU.

The brute-force cases use integer-valued one-channel frames: every distance and every path cost is an exact small integer, so
"the minimum" and "a tie" mean the same thing to the recurrence and to the enumeration."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import dtw_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,m", list(itertools.product(range(1, 6), range(1, 6))))
def test_restatement_is_the_minimum_over_all_paths(n, m):
    rng = np.random.default_rng(100 * n + m)
    for spread in (1, 4):                                          # spread 1: almost everything ties, the order decides
        for _ in range(6):
            p = rng.integers(-spread, spread + 1, size=(n, 1)).astype(np.float32)
            q = rng.integers(-spread, spread + 1, size=(m, 1)).astype(np.float32)
            got = ref.dtw(p, q)
            cost, steps = ref.brute_force(ref.distances(p, q))
            assert got["cost"] == cost and got["steps"] == steps, (p.ravel(), q.ravel())
            assert max(n, m) <= got["steps"] <= n + m - 1 and got["E"] == 0.0


def test_restatement_on_sequences_worked_by_hand():
    def run(x, y):
        r = ref.dtw(np.array(x, dtype=np.float32)[:, None], np.array(y, dtype=np.float32)[:, None])
        return r["cost"], r["steps"]
    assert run([0, 1, 2], [0, 2]) == (1.0, 3)                      # D(1,1) = 1 by the diagonal, D(2,1) = 0 + D(1,0) by the diagonal
    assert run([1, 2, 3, 4], [1, 1, 2, 3, 3, 4]) == (0.0, 6)      # one path of cost 0: it repeats the 1 and the 3
    assert run([0, 0], [3]) == (6.0, 2)
    assert run([5], [5]) == (0.0, 1)
    assert run([0] * 4, [0] * 7) == (0.0, 7)                       # all paths tie: diagonal first gives max(N, M) steps
    assert run([0] * 7, [0] * 4) == (0.0, 7)


def test_cepstral_basis_is_the_scaled_orthonormal_dct_without_its_first_row():
    from reformer_tts_amd import evaluation
    for n_mel, n_coef in ((80, 13), (20, 19), (7, 3)):
        basis = evaluation.cepstral_basis(n_mel, n_coef)
        assert basis.dtype == torch.float32 and tuple(basis.shape) == (n_coef, n_mel)
        scale = 10.0 / np.log(10.0) * np.sqrt(2.0)
        rows = basis.double().numpy() / scale
        assert np.abs(rows @ rows.T - np.eye(n_coef)).max() < 1e-6                    # orthonormal before the dB scale (f32 entries)
        assert np.abs(rows.sum(axis=1)).max() < 1e-5                                  # no k = 0 row: every row is orthogonal to a constant
        assert np.array_equal(basis.numpy(), ref.cepstral_basis(n_mel, n_coef).astype(np.float32))
        k, m = 1, 0
        assert abs(rows[0, 0] - np.sqrt(2.0 / n_mel) * np.cos(np.pi * k * (m + 0.5) / n_mel)) < 1e-7
    with pytest.raises(ValueError, match="n_coef"):
        evaluation.cepstral_basis(13, 13)


def test_the_three_symbols_are_declared_and_exported():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtts.h")).read(), flags=re.S)
    for name in ("rtts_dtw_align", "rtts_dtw_max_frames", "rtts_dtw_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        proto = re.search(name + r"\s*\(([^)]*)\)", header).group(1).strip()
        count = 0 if proto in ("", "void") else len(proto.split(","))
        assert count == len(_lib.SIGNATURES[name]), name
    assert lib.rtts_dtw_max_frames() >= 2048
    most = lib.rtts_dtw_max_frames()
    assert lib.rtts_dtw_workspace_bytes(12, 1024, 1020, 13) > 12 * 1024 * 1020 * 4    # at least the distance tables
    assert lib.rtts_dtw_workspace_bytes(1, most, most, 128) > 0
    for bad in ((0, 8, 8, 13), (1, most + 1, 8, 13), (1, 8, most + 1, 13), (1, 8, 0, 13), (1, 8, 8, 129), (1, -1, 8, 13)):
        assert lib.rtts_dtw_workspace_bytes(*bad) == -1, bad


def test_the_entry_point_refuses_by_name_before_any_launch():
    """Every argument set here ends at a check: the base set's workspace is too small, the last thing the entry point looks at, so
    nothing is launched even where a change goes unnoticed (the pointers are made up)."""
    from reformer_tts_amd import _lib
    lib = _lib.load()
    most = lib.rtts_dtw_max_frames()
    good = dict(gen=64, gs_b=0, gs_mel=1, gs_t=1, L=8, gen_stop=None, truth=64, ts_mel=1, ts_t=1, truth_frames=8, fo=None, n_utt=0, ids=None,
                starts=64, lengths=64, B=1, n_mel=1, lm=8, basis=None, n_proj=1, work=64, work_bytes=16, phases=15, cost=64, steps=64,
                totals=64, stream=None)
    for change, word in ((dict(L=most + 1), "L must be"), (dict(lm=most + 1), "lm must be"), (dict(lm=0), "lm must be"),
                         (dict(fo=64), "two truth descriptions"), (dict(starts=None, lengths=None), "no truth description"),
                         (dict(lengths=None), "both starts and lengths"), (dict(n_proj=2), "n_proj must be n_mel"),
                         (dict(n_mel=129, n_proj=129), "n_mel must be"), (dict(), "workspace_bytes"), (dict(phases=0), "phases"),
                         (dict(B=0), "B must be"), (dict(cost=None), "cost is a null")):
        args = dict(good)
        args.update(change)
        with pytest.raises(_lib.RttsError, match=word):
            _lib.call("rtts_dtw_align", *args.values())


def test_ops_refuses_bad_arguments_on_the_host():
    from reformer_tts_amd import _lib, ops
    gen, stop, truth = torch.zeros(2, 7, 5), torch.zeros(2, dtype=torch.int64), torch.zeros(7, 20)
    fo, ids = torch.tensor([0, 8, 20]), torch.tensor([1, 0], dtype=torch.int32)
    starts, lengths = torch.tensor([0, 8]), torch.tensor([8, 12], dtype=torch.int32)
    with pytest.raises(ValueError, match="exactly one"):                      # neither description
        ops.dtw_align(gen, stop, truth, 12)
    with pytest.raises(ValueError, match="exactly one"):                      # both
        ops.dtw_align(gen, stop, truth, 12, frame_offsets=fo, ids=ids, starts=starts, lengths=lengths)
    with pytest.raises(ValueError, match="exactly one"):                      # half of the padded-batch description
        ops.dtw_align(gen, stop, truth, 12, starts=starts)
    with pytest.raises(ValueError, match="exactly one"):                      # ids belong to the corpus description
        ops.dtw_align(gen, stop, truth, 12, ids=ids, starts=starts, lengths=lengths)
    for bad in (dict(gen=gen.double()), dict(gen_stop=stop.int()), dict(truth=truth.half())):
        args = dict(gen=gen, gen_stop=stop, truth=truth)
        args.update(bad)
        with pytest.raises(ValueError, match="must be a torch"):
            ops.dtw_align(args["gen"], args["gen_stop"], args["truth"], 12, frame_offsets=fo, ids=ids)
    with pytest.raises(ValueError, match="basis must be a torch.float32"):
        ops.dtw_align(gen, stop, truth, 12, frame_offsets=fo, ids=ids, basis=torch.zeros(3, 7, dtype=torch.float64))
    with pytest.raises(ValueError, match="lengths must be a torch.int32"):
        ops.dtw_align(gen, stop, truth, 12, starts=starts, lengths=lengths.long())
    with pytest.raises(_lib.RttsError, match="GPU only"):                     # everything right but the device
        ops.dtw_align(gen, stop, truth, 12, frame_offsets=fo, ids=ids)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        ops.dtw_align(gen, None, truth, 12, starts=starts, lengths=lengths, basis=torch.zeros(3, 7))
    assert ops.dtw_max_frames() >= 2048
