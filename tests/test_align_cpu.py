"""Host-side checks of the alignment path: the float64 restatement of tests/align_ref.py against brute-force enumeration of every
monotonic surjective path and against cases worked by hand, the declarations of the new symbols, and the argument checks of the
two entry points and their Python wrappers (dummy pointers, no launch, no GPU)."""
import math
import os

import numpy as np
import pytest
import torch

import align_ref as ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_mas_restatement_against_every_path(k):
    """All T <= 8 for this K <= 4, three random matrices each: the best score over every monotonic surjective path, and the
    back-tracked path is one of the best."""
    for t in range(k, 9):
        for seed in range(3):
            a = ref.pure_noise(t, k, 100 * t + 10 * k + seed)
            dur, path, scores, margin = ref.mas_ref(a, t, k)
            best, paths = ref.mas_brute_force(a, t, k)
            assert abs(scores[0] - best) <= 1e-12 * max(1.0, abs(best)), (t, k, seed)
            assert tuple(int(p) for p in path[:t]) in paths
            assert dur[:k].min() >= 1 and dur.sum() == t and path[0] == 0 and path[t - 1] == k - 1
            assert np.all(np.diff(path[:t]) >= 0) and np.all(np.diff(path[:t]) <= 1)
            assert scores[1] == sum(float(a[i, path[i]]) for i in range(t))
            assert margin > 0


@pytest.mark.parametrize("t,k,want", [(10, 4, [1, 1, 1, 7]), (4, 4, [1, 1, 1, 1]), (64, 3, [1, 1, 62])])
def test_mas_on_a_constant_matrix_stays_on_every_tie(t, k, want):
    dur, path, scores, margin = ref.mas_ref(ref.constant(t, k), t, k)
    assert dur.tolist() == want
    assert margin == 0.0 or t == k                             # every open decision is an exact tie
    assert scores[0] == sum([math.log(2.0 ** -7)] * t) and scores[1] == t * 2.0 ** -7


def test_mas_on_an_identity_like_matrix_and_beyond_its_region():
    a = (0.9 * np.eye(6) + 0.1 / 6).astype(np.float32)
    dur, path, _, _ = ref.mas_ref(a, 6, 6)
    assert dur.tolist() == [1] * 6 and path.tolist() == list(range(6))
    wide = np.full((9, 8), np.nan, dtype=np.float32)           # a NaN outside the region changes nothing
    wide[:6, :6] = a
    dur, path, scores, _ = ref.mas_ref(wide, 6, 6)
    assert dur.tolist() == [1] * 6 + [0, 0] and path.tolist() == list(range(6)) + [-1] * 3 and np.isfinite(scores).all()
    for t, k in ((0, 3), (10, 3), (3, 9), (2, 3)):             # no frame, too many frames / keys, fewer frames than keys
        dur, path, scores, _ = ref.mas_ref(wide, t, k)
        assert not dur.any() and (path == -1).all() and np.isnan(scores).all()
    wide[2, 3] = np.inf
    assert np.isnan(ref.mas_ref(wide, 6, 6)[2]).all()


def test_stats_by_hand():
    a = np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]], dtype=np.float32)
    argmax, dur, row = ref.stats_ref(a, 3, 3, 0.2)
    w1, w2 = 1 - math.exp(-(1 / 9) / 0.08), 1 - math.exp(-(4 / 9) / 0.08)
    assert argmax.tolist() == [0, 1, 2] and dur.tolist() == [1, 1, 1]
    assert row[:4].tolist() == [3, 3, 3.0, 1.5] and row[6:].tolist() == [2, 3]
    np.testing.assert_allclose(row[4], 4.5 * math.log(2), rtol=1e-14)
    np.testing.assert_allclose(row[5], w1 + 0.5 * w2, rtol=1e-14)
    tie = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]], dtype=np.float32)
    argmax, dur, row = ref.stats_ref(tie, 3, 3, 0.2)           # the lowest index wins; 0 ln 0 counts as 0; the track falls back once
    assert argmax.tolist() == [0, 1, 0] and dur.tolist() == [2, 1, 0] and row[6:].tolist() == [1, 2]
    np.testing.assert_allclose(row[4], 3 * math.log(2), rtol=1e-14)
    argmax, dur, row = ref.stats_ref(tie, 2, 1, 0.2)           # a sub-region: one key
    assert argmax.tolist() == [0, 0, -1] and dur.tolist() == [2, 0, 0] and row.tolist() == [2, 1, 0.5, 0.5, row[4], 0.0, 1, 1]
    for t, k in ((0, 3), (4, 3), (3, 4)):
        argmax, dur, row = ref.stats_ref(tie, t, k, 0.2)
        assert (argmax == -1).all() and not dur.any() and np.isnan(row).all()


def test_generators():
    d = ref.dyadic(20, 40, 20, 33, 1)
    assert d.shape == (20, 40) and np.all(d[:, :33] * 1024 == np.round(d[:, :33] * 1024)) and np.all(d[:, :33].astype(np.float64).sum(1) == 1.0)
    assert not d[:, 33:].any()
    n = ref.noisy_diagonal(30, 20, 25, 17, 60.0, 0.5, 2)
    np.testing.assert_allclose(n[:25, :17].sum(1), 1.0, rtol=1e-6)
    assert not n[25:].any() and not n[:, 17:].any()
    assert ref.pure_noise(5, 7, 0).shape == (5, 7) and ref.constant(3, 4).tolist() == [[2.0 ** -7] * 4] * 3


# ------------------------------------------------------------------ declarations and refusals
def test_header_and_signatures_hold_the_new_symbols(lib):
    from reformer_tts_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rtts.h")).read()
    for name in ("rtts_align_stats", "rtts_align_mas", "rtts_align_stats_workspace", "rtts_align_mas_workspace"):
        assert f"{name}(" in text and hasattr(lib, name) and name in _lib.SIGNATURES


def test_workspace_sizes(lib):
    assert lib.rtts_align_mas_workspace(3, 12, 1024, 256) > 0              # the validation shape: back-pointers in LDS
    assert lib.rtts_align_mas_workspace(3, 12, 1024, 256) < 4096
    assert lib.rtts_align_mas_workspace(1, 1, 4096, 512) >= 4096 * 512 // 8     # one bit per cell in the workspace
    assert lib.rtts_align_mas_workspace(2, 3, 4096, 2048) >= 6 * 4096 * 2048 // 8
    assert lib.rtts_align_stats_workspace(3, 12, 1024, 256) > 0
    for fn in (lib.rtts_align_stats_workspace, lib.rtts_align_mas_workspace):
        for bad in ((0, 1, 8, 8), (65, 1, 8, 8), (1, 0, 8, 8), (1, 65536, 8, 8), (1, 1, 0, 8), (1, 1, 4097, 8), (1, 1, 8, 0), (1, 1, 8, 2049)):
            assert fn(*bad) == -1, bad


def _call(lib, entry, **kw):
    """One of the two entries with dummy (never dereferenced) pointers: every case here must be rejected before a launch."""
    n_mat, b, tq, tk = kw.get("n_mat", 2), kw.get("B", 3), kw.get("Tq", 64), kw.get("Tk", 32)
    st = kw.get("st", 32)
    sb = kw.get("sb", tq * st)
    sm = kw.get("sm", 3 * sb)
    args = dict(a=kw.get("a", 4096), sm=sm, sb=sb, st=st, n_mat=n_mat, B=b, Tq=tq, Tk=tk, n_frames=64, n_keys=64,
                scalar=kw.get("scalar", 0.2), out0=64, out1=64, out2=64, workspace=64, workspace_bytes=kw.get("workspace_bytes", 1 << 40),
                stream=None)
    if "null" in kw:
        args[kw["null"]] = None
    rc = getattr(lib, entry)(*args.values())
    return rc, lib.rtts_last_error().decode()


BAD = [
    (dict(null="a"), "a is a null"), (dict(null="n_frames"), "n_frames is a null"), (dict(null="n_keys"), "n_keys is a null"),
    (dict(null="out0"), "null"), (dict(null="out2"), "null"), (dict(null="workspace"), "workspace is a null"),
    (dict(a=4100), "16-byte aligned"), (dict(a=4104), "16-byte aligned"),
    (dict(st=34), "st"), (dict(st=28), "st"), (dict(sb=64 * 32 + 2), "sb"), (dict(sm=3 * 64 * 32 + 1), "sm"), (dict(sb=-2048), "sb"),
    (dict(sb=63 * 32), "overlap"), (dict(sm=2 * 64 * 32), "overlap"), (dict(sm=64 * 32, sb=64 * 32), "overlap"),
    (dict(Tq=0), "Tq"), (dict(Tq=4097), "Tq"), (dict(Tk=0), "Tk"), (dict(Tk=2049, st=2052), "Tk"),
    (dict(n_mat=0), "n_mat"), (dict(n_mat=65), "n_mat"), (dict(B=0), "B must"), (dict(B=65536), "B must"),
    (dict(workspace_bytes=0), "workspace_bytes"),
]


@pytest.mark.parametrize("kw,word", BAD + [(dict(null="out1"), "dur_argmax is a null"), (dict(scalar=0.0), "sigma"),
                                           (dict(scalar=-0.2), "sigma"), (dict(scalar=float("nan")), "sigma"),
                                           (dict(scalar=float("inf")), "sigma")])
def test_stats_rejects_bad_arguments_without_a_launch(lib, kw, word):
    rc, msg = _call(lib, "rtts_align_stats", **kw)
    assert rc != 0 and "rtts_align_stats" in msg and word in msg, msg


@pytest.mark.parametrize("kw,word", BAD + [(dict(scalar=0.0), "floor"), (dict(scalar=-1e-30), "floor"), (dict(scalar=float("nan")), "floor"),
                                           (dict(Tq=4096, Tk=512, st=512, workspace_bytes=4096 * 512 // 8 - 1), "workspace_bytes")])
def test_mas_rejects_bad_arguments_without_a_launch(lib, kw, word):
    rc, msg = _call(lib, "rtts_align_mas", **kw)
    assert rc != 0 and "rtts_align_mas" in msg and word in msg, msg


def test_wrappers_refuse_cpu_tensors_and_wrong_types_by_name(lib):
    from reformer_tts_amd import _lib, evaluation, ops
    mats = torch.zeros(2, 3, 8, 8)
    nf, nk = torch.full((3,), 8, dtype=torch.int32), torch.full((3,), 8, dtype=torch.int32)
    for fn in (ops.alignment_stats, ops.alignment_mas):
        with pytest.raises(_lib.RttsError, match="runs on the GPU only: mats"):
            fn(mats, nf, nk)
        with pytest.raises(_lib.RttsError, match="runs on the GPU only: mats"):
            fn([mats[0], mats[1]], nf, nk)
        with pytest.raises(_lib.RttsError, match="mats must be a CUDA torch.float32"):
            fn(mats.double(), nf, nk)
        with pytest.raises(ValueError, match="empty"):
            fn([], nf, nk)
    with pytest.raises(ValueError, match="sigma"):
        ops.alignment_stats(mats, nf, nk, sigma=0.0)
    with pytest.raises(ValueError, match="floor"):
        ops.alignment_mas(mats, nf, nk, floor=0.0)
    with pytest.raises(_lib.RttsError, match="alignment_stats runs on the GPU only"):
        evaluation.alignment_scores(mats, nf.long(), nk.long())
    with pytest.raises(_lib.RttsError, match="alignment_mas runs on the GPU only"):
        evaluation.alignment_durations(mats, nf, nk)
