"""``rtts_dtw_align`` on the GPU against its float64 restatement (tests/dtw_ref.py).

Exact cases: no basis, integer-valued frames in one channel -- every difference, square, square root and partial path sum is a
small integer, exact in f32 and f64 in any order -- so cost and steps must EQUAL the reference, ties included.

Random cases: the reference runs on its OWN projected f32 frames (the kernel's projection is held to them separately), so what
is left to differ is the f32 frame distance: a sum of n_proj squared differences under a square root, each term within 3 * 2^-24
relative (subtraction, square), the sum of positive terms within n_proj * 2^-24 more in any order, the root half of that plus its
own rounding: below (n_proj + 4) * 2^-23 relative.  A path cost is a sum of such positive distances and inherits the worst
term's relative error (the f64 additions are far below).  ``steps`` is a discrete function of the table: it is compared only
where the reference's margin -- the smallest gap along its optimal path between the chosen predecessor and the runner-up --
exceeds 8 E, E being the largest difference between the float64 table and the one from f32-rounded distances (8 for another
summation order than the rounding E sees); at most one case in ten may be left out that way.

In every batch here the generated frames past N_b and the truth frames past M_b are NaN: a result is the proof they were not read."""
import numpy as np
import pytest
import torch

import dtw_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -23


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _pack(gens, truths, gpu, frames=None, lm=None, gap=3):
    """-> dict of device tensors: gen (B, n_mel, L) NaN past N_b with gen_stop, the truths end to end (n_mel, total) with ``gap`` NaN
    frames between them, and the two descriptions of where they lie."""
    n_mel = gens[0].shape[0]
    frames = frames or max(g.shape[1] for g in gens)
    gen = np.full((len(gens), n_mel, frames), np.nan, dtype=np.float32)
    for b, g in enumerate(gens):
        gen[b, :, :g.shape[1]] = g
    offs, cols = [0], []
    for t in truths:
        cols += [t, np.full((n_mel, gap), np.nan, dtype=np.float32)]
        offs.append(offs[-1] + t.shape[1] + gap)
    truth = np.concatenate(cols, axis=1)
    lens = [t.shape[1] for t in truths]
    return dict(gen=torch.from_numpy(gen).to(gpu), stop=torch.tensor([g.shape[1] for g in gens], dtype=torch.int64).to(gpu),
                truth=torch.from_numpy(truth).to(gpu), starts=torch.tensor(offs[:-1], dtype=torch.int64).to(gpu),
                lengths=torch.tensor(lens, dtype=torch.int32).to(gpu), lm=lm or max(lens))


def _run(pk, basis=None, **kw):
    from reformer_tts_amd import ops
    cost, steps, totals = ops.dtw_align(pk["gen"], pk["stop"], pk["truth"], pk["lm"], basis=basis, starts=pk["starts"], lengths=pk["lengths"], **kw)
    return cost.cpu().numpy(), steps.cpu().numpy(), totals.cpu().numpy()


def _ints(rng, n, spread=3):
    return rng.integers(-spread, spread + 1, size=(1, n)).astype(np.float32)


def test_textbook_sequences(gpu):
    """Worked by hand (the same cases tests/test_dtw_cpu.py holds the restatement to)."""
    cases = [([0, 1, 2], [0, 2], 1.0, 3), ([1, 2, 3, 4], [1, 1, 2, 3, 3, 4], 0.0, 6), ([0, 0], [3], 6.0, 2), ([5], [5], 0.0, 1),
             ([0] * 4, [0] * 7, 0.0, 7), ([0] * 7, [0] * 4, 0.0, 7)]
    gens = [np.array(c[0], dtype=np.float32)[None, :] for c in cases]
    truths = [np.array(c[1], dtype=np.float32)[None, :] for c in cases]
    cost, steps, totals = _run(_pack(gens, truths, gpu))
    assert cost.tolist() == [c[2] for c in cases] and steps.tolist() == [c[3] for c in cases]
    want = np.array([c[2] for c in cases])
    assert totals[0] == np.mean(want / steps) and totals[1] == want.sum() / steps.sum()


SIZES = (1, 2, 63, 64, 65, 257)


@pytest.mark.parametrize("kind", ["integers", "constant"])
def test_every_size_exactly(gpu, kind):
    """N and M from SIZES in every combination plus 1 x 300 and 300 x 1, one batch.  Constant sequences: every path costs 0, so
    steps is max(N, M) only if the diagonal is tried first and replaced on strict < alone."""
    rng = np.random.default_rng(11)
    shapes = [(n, m) for n in SIZES for m in SIZES] + [(1, 300), (300, 1)]
    if kind == "integers":
        gens, truths = [_ints(rng, n) for n, _ in shapes], [_ints(rng, m) for _, m in shapes]
    else:
        gens, truths = [np.full((1, n), 2.0, dtype=np.float32) for n, _ in shapes], [np.full((1, m), 2.0, dtype=np.float32) for _, m in shapes]
    cost, steps, totals = _run(_pack(gens, truths, gpu))
    want_cost, want_steps, want_totals, _ = ref.align(gens, truths)
    assert np.array_equal(cost, want_cost) and np.array_equal(steps, want_steps)
    assert all(max(n, m) <= s <= n + m - 1 for (n, m), s in zip(shapes, steps))
    if kind == "constant":
        assert np.all(cost == 0.0) and steps.tolist() == [max(n, m) for n, m in shapes]
    np.testing.assert_allclose(totals, want_totals, rtol=1e-14)


def test_two_rows_per_thread_exactly(gpu):
    """More than 1024 generated frames put two table rows on a thread: integer sequences again, around that threshold."""
    rng = np.random.default_rng(12)
    shapes = [(1025, 70), (1300, 1111), (1024, 1024)]
    gens, truths = [_ints(rng, n) for n, _ in shapes], [_ints(rng, m) for _, m in shapes]
    for pick in ([0, 1], [2]):                                     # L = 1300: two rows; L = 1024: one row, all 16 waves
        g, t = [gens[i] for i in pick], [truths[i] for i in pick]
        cost, steps, _ = _run(_pack(g, t, gpu))
        want_cost, want_steps, _, _ = ref.align(g, t)
        assert np.array_equal(cost, want_cost) and np.array_equal(steps, want_steps)


@pytest.mark.parametrize("with_basis", [False, True], ids=["mel", "cepstra"])
def test_identical_sequences_cost_exactly_zero(gpu, with_basis):
    """The |p|^2 + |q|^2 - 2 p.q form of the distance leaves rounding dust here; the difference form leaves 0.0."""
    from reformer_tts_amd import evaluation
    rng = np.random.default_rng(13)
    seqs = [(-5 + 2 * rng.standard_normal((80, n))).astype(np.float32) for n in (1, 77, 200)]
    basis = evaluation.cepstral_basis(80, 13, gpu) if with_basis else None
    cost, steps, totals = _run(_pack(seqs, seqs, gpu), basis)
    assert cost.tolist() == [0.0, 0.0, 0.0] and steps.tolist() == [1, 77, 200] and totals.tolist() == [0.0, 0.0]


@pytest.fixture(scope="module")
def warped():
    rng = np.random.default_rng(2024)
    cases = [ref.warped_case(rng) for _ in range(10)]
    return [c[0] for c in cases], [c[1] for c in cases]


@pytest.mark.parametrize("with_basis", [False, True], ids=["mel", "cepstra"])
def test_warped_sequences_against_float64(gpu, warped, with_basis):
    from reformer_tts_amd import evaluation, ops
    gens, truths = warped
    basis = evaluation.cepstral_basis(80, 13, gpu) if with_basis else None
    host_basis = None if basis is None else basis.cpu().numpy()
    n_proj = 13 if with_basis else 80
    pk = _pack(gens, truths, gpu)
    b, frames = len(gens), pk["gen"].shape[2]
    lib_bytes = ops._lib.load().rtts_dtw_workspace_bytes(b, frames, pk["lm"], n_proj)
    out = torch.empty(b + 2, dtype=torch.float64, device=gpu)
    state = (torch.empty(lib_bytes, dtype=torch.uint8, device=gpu), out[:b], torch.empty(b, dtype=torch.int32, device=gpu), out[b:])
    cost, steps, totals = _run(pk, basis, _state=state)
    want_cost, want_steps, want_totals, slots = ref.align(gens, truths, host_basis)
    # the kernel's projection: the workspace begins with the projected generated frames, f32 (B, L, n_proj) (include/rtts.h)
    proj = state[0][:b * frames * n_proj * 4].view(torch.float32).view(b, frames, n_proj).cpu().numpy()
    worst_proj = 0.0
    for i, g in enumerate(gens):
        want = ref.project(g, host_basis)
        ulp = np.spacing(np.abs(want).max(axis=1, keepdims=True).astype(np.float32)).astype(np.float64)
        worst_proj = max(worst_proj, float((np.abs(proj[i, :g.shape[1]].astype(np.float64) - want) / ulp).max()))
    rel = np.abs(cost - want_cost) / want_cost
    clear = np.array([s["margin"] > 8 * s["E"] for s in slots])
    print(f"\n[dtw warped, n_proj {n_proj}] cost rel err max {rel.max():.3e} (bound {(n_proj + 4) * U:.3e}); projection off by {worst_proj:.2f} ulp "
          f"of the frame's largest coefficient (bound 2); smallest margin {min(s['margin'] for s in slots):.3e}, largest E "
          f"{max(s['E'] for s in slots):.3e}; steps compared in {int(clear.sum())} of {b}, equal in {int((steps == want_steps)[clear].sum())}")
    assert worst_proj <= 2.0
    assert np.all(rel <= (n_proj + 4) * U)
    assert (~clear).sum() <= b // 10
    assert np.array_equal(steps[clear], want_steps[clear])
    if clear.all():
        np.testing.assert_allclose(totals, want_totals, rtol=(n_proj + 4) * U)


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(5)
    shapes = [(90, 120), (200, 64), (33, 33), (130, 257)]
    gens = [(-5 + 2 * rng.standard_normal((80, n))).astype(np.float32) for n, _ in shapes]
    truths = [(-5 + 2 * rng.standard_normal((80, m))).astype(np.float32) for _, m in shapes]
    return gens, truths


def _bits(result):
    return [r.tobytes() for r in result]


def test_layouts_and_descriptions_give_the_same_bits(gpu, ragged):
    from reformer_tts_amd import evaluation, ops
    gens, truths = ragged
    pk = _pack(gens, truths, gpu)
    for basis in (None, evaluation.cepstral_basis(80, 13, gpu)):
        first = _run(pk, basis)
        assert _bits(_run(pk, basis)) == _bits(first)                                          # a second call
        gen_t = pk["gen"].transpose(1, 2).contiguous()                                         # (B, T, n_mel)
        assert _bits(_run(dict(pk, gen=gen_t), basis, gen_frames_last=False)) == _bits(first)
        truth_t = pk["truth"].t().contiguous()                                                 # (frames, n_mel) rows
        assert _bits(_run(dict(pk, gen=gen_t, truth=truth_t), basis, gen_frames_last=False, truth_frames_last=False)) == _bits(first)
        # the corpus description: the same frames named by offsets and ids, the gaps as utterances of their own, out of order
        bounds = []
        for s, n in zip(pk["starts"].tolist(), pk["lengths"].tolist()):
            bounds += [s, s + n]
        fo = torch.tensor(bounds + [pk["truth"].shape[1]], dtype=torch.int64).to(gpu)
        ids = torch.tensor([0, 2, 4, 6], dtype=torch.int32).to(gpu)
        got = ops.dtw_align(pk["gen"], pk["stop"], pk["truth"], pk["lm"], basis=basis, frame_offsets=fo, ids=ids)
        assert _bits([t.cpu().numpy() for t in got]) == _bits(first)
        swapped = ops.dtw_align(pk["gen"][[1, 0, 2, 3]], pk["stop"][[1, 0, 2, 3]], pk["truth"], pk["lm"] + 40, basis=basis, frame_offsets=fo,
                                ids=torch.tensor([2, 0, 4, 6], dtype=torch.int32).to(gpu))
        assert torch.equal(swapped[0].cpu()[[1, 0, 2, 3]], torch.from_numpy(first[0]))        # a slot does not depend on its place or on lm
        want_cost, _, _, _ = ref.align(gens, truths, None if basis is None else basis.cpu().numpy())
        np.testing.assert_allclose(first[0], want_cost, rtol=((80 if basis is None else 13) + 4) * U)


def test_graph_replay_gives_the_eager_bits(gpu, ragged):
    from reformer_tts_amd import evaluation, ops
    pk = _pack(*ragged, gpu)
    basis = evaluation.cepstral_basis(80, 13, gpu)
    eager = _run(pk, basis)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.dtw_align(pk["gen"], pk["stop"], pk["truth"], pk["lm"], basis=basis, starts=pk["starts"], lengths=pk["lengths"])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.dtw_align(pk["gen"], pk["stop"], pk["truth"], pk["lm"], basis=basis, starts=pk["starts"], lengths=pk["lengths"])
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _bits([t.cpu().numpy() for t in out]) == _bits(eager)
    pk["stop"][1] = 150                                            # the lengths are read on the device: a replay follows them
    graph.replay()
    torch.cuda.synchronize()
    want = _run(pk, basis)
    assert _bits([t.cpu().numpy() for t in out]) == _bits(want) and want[0][1] != eager[0][1]


def test_gen_stop_moves_only_its_own_slot(gpu, ragged):
    gens, truths = ragged
    pk = _pack(gens, truths, gpu)
    pk["gen"] = torch.nan_to_num(pk["gen"], nan=-5.0)                # frames past N_b are now readable: a longer stop reads them
    base = _run(pk)
    for b, stop in ((0, 60), (1, 10_000), (3, 131), (2, 1)):
        changed = dict(pk, stop=pk["stop"].clone())
        changed["stop"][b] = stop
        cost, steps, _ = _run(changed)
        others = [i for i in range(4) if i != b]
        assert np.array_equal(cost[others], base[0][others]) and np.array_equal(steps[others], base[1][others])
        n = min(stop, pk["gen"].shape[2])
        want = ref.align([pk["gen"][b, :, :n].cpu().numpy()], [truths[b]])
        np.testing.assert_allclose(cost[b], want[0][0], rtol=(80 + 4) * U)
    no_stop = ops_no_stop(pk)
    want = ref.align([pk["gen"][b].cpu().numpy() for b in range(4)], truths)
    np.testing.assert_allclose(no_stop, want[0], rtol=(80 + 4) * U)          # gen_stop = None: all L frames


def ops_no_stop(pk):
    from reformer_tts_amd import ops
    return ops.dtw_align(pk["gen"], None, pk["truth"], pk["lm"], starts=pk["starts"], lengths=pk["lengths"])[0].cpu().numpy()


def test_slots_that_cannot_be_scored_are_nan(gpu, ragged):
    from reformer_tts_amd import ops
    gens, truths = ragged
    pk = _pack(gens, truths, gpu)
    base = _run(pk)
    assert np.all(np.isfinite(base[0])) and np.all(np.isfinite(base[2]))      # NaN beyond N_b and M_b (the packing) reached nothing

    def only(b, cost, steps, totals):
        others = [i for i in range(4) if i != b]
        assert np.isnan(cost[b]) and steps[b] == 0 and np.all(np.isnan(totals))
        assert np.array_equal(cost[others], base[0][others]) and np.array_equal(steps[others], base[1][others])

    for where in ("gen", "truth"):                                            # a non-finite value in a compared frame
        for value in (float("nan"), float("inf")):
            poisoned = dict(pk)
            poisoned[where] = pk[where].clone()
            if where == "gen":
                poisoned["gen"][2, 17, 32] = value                            # slot 2's last compared frame
            else:
                poisoned["truth"][40, int(pk["starts"][1]) + 5] = value
            only(2 if where == "gen" else 1, *_run(poisoned))
    empty = dict(pk, stop=pk["stop"].clone())
    empty["stop"][3] = 0                                                      # N_b = 0
    only(3, *_run(empty))
    outside = dict(pk, lengths=pk["lengths"].clone())
    outside["lengths"][3] = 400                                               # leaves [0, truth_frames]
    only(3, *_run(outside))
    fo = torch.tensor([0, 120, 123, 187], dtype=torch.int64).to(gpu)
    for bad_id in (-1, 3):                                                    # an id outside [0, n_utt)
        ids = torch.tensor([0, 2, bad_id, 0], dtype=torch.int32).to(gpu)
        cost, steps, totals = [t.cpu().numpy() for t in ops.dtw_align(pk["gen"], pk["stop"], pk["truth"], pk["lm"], frame_offsets=fo, ids=ids)]
        assert np.isnan(cost[2]) and steps[2] == 0 and np.all(np.isnan(totals)) and np.array_equal(cost[:2], base[0][:2])


def test_a_zero_length_truth_scores_nothing_or_cannot_be_scored(gpu):
    """The one place where the two users of the shared truth pick (csrc/score_common.h) differ: a slot whose truth has no frame is
    a valid slot of 0 frames for infer_metrics (sse 0, stop_err = |gen_stop - (0 - 1)|) and an unscorable one for dtw_align
    (cost NaN, steps 0, totals NaN).  Either way the other slots keep their bits."""
    from reformer_tts_amd import ops
    rng = np.random.default_rng(31)
    b, n_mel, frames, lm = 3, 7, 40, 50
    gens = [(-5 + 2 * rng.standard_normal((n_mel, frames))).astype(np.float32) for _ in range(b)]
    truths = [(-5 + 2 * rng.standard_normal((n_mel, m))).astype(np.float32) for m in (33, 21, 45)]
    pk = _pack(gens, truths, gpu, frames=frames, lm=lm)
    pk["stop"] = torch.tensor([40, 17, 38], dtype=torch.int64).to(gpu)
    empty = dict(pk, lengths=pk["lengths"].clone())
    empty["lengths"][1] = 0

    def metrics(p):
        return [t.cpu().numpy() for t in ops.infer_metrics(p["gen"], p["stop"], p["truth"], p["lm"], starts=p["starts"], lengths=p["lengths"])]

    (sse0, err0, tot0), (sse1, err1, tot1) = metrics(pk), metrics(empty)
    assert np.all(np.isfinite(sse0)) and sse0[1] > 0.0 and np.all(np.isfinite(tot0))
    assert sse1[1] == 0.0 and err1[1] == 17 + 1 and np.all(np.isfinite(tot1))
    assert _bits([sse1[[0, 2]], err1[[0, 2]]]) == _bits([sse0[[0, 2]], err0[[0, 2]]])
    (cost0, steps0, dtot0), (cost1, steps1, dtot1) = _run(pk), _run(empty)
    assert np.all(np.isfinite(cost0)) and np.all(steps0 > 0) and np.all(np.isfinite(dtot0))
    assert np.isnan(cost1[1]) and steps1[1] == 0 and np.all(np.isnan(dtot1))
    assert _bits([cost1[[0, 2]], steps1[[0, 2]]]) == _bits([cost0[[0, 2]], steps0[[0, 2]]])


def test_sizes_past_the_limit_are_refused_by_name(gpu):
    from reformer_tts_amd import _lib, ops
    most = ops.dtw_max_frames()
    assert most >= 2048
    gen, truth = torch.zeros(1, 4, most + 1, device=gpu), torch.zeros(4, most + 1, device=gpu)
    where = dict(starts=torch.zeros(1, dtype=torch.int64, device=gpu), lengths=torch.full((1,), 8, dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError, match="L = "):
        ops.dtw_align(gen, None, truth, 8, **where)
    with pytest.raises(ValueError, match="lm = "):
        ops.dtw_align(gen[:, :, :8], None, truth, most + 1, **where)
    with pytest.raises(ValueError, match="exactly one"):
        ops.dtw_align(gen[:, :, :8], None, truth, 8)
    with pytest.raises(ValueError, match="exactly one"):
        ops.dtw_align(gen[:, :, :8], None, truth, 8, frame_offsets=torch.tensor([0, 8], device=gpu), **where)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    out = torch.full((4,), 7.0, dtype=torch.float64, device=gpu)
    with pytest.raises(_lib.RttsError, match="L must be"):                    # the entry point itself, past ops' own check
        _lib.call("rtts_dtw_align", gen.data_ptr(), gen.stride(0), gen.stride(1), 1, most + 1, None, truth.data_ptr(), truth.stride(0), 1,
                  most + 1, None, 0, None, where["starts"].data_ptr(), where["lengths"].data_ptr(), 1, 4, 8, None, 4, work.data_ptr(), work.numel(),
                  15, out.data_ptr(), work.data_ptr(), out[2:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert out.tolist() == [7.0] * 4                                          # nothing was launched


def test_the_largest_single_slot(gpu):
    """rtts_dtw_max_frames() generated frames against as many truth frames, 80 mels through the cepstral basis, once."""
    from reformer_tts_amd import evaluation, ops
    most = ops.dtw_max_frames()
    rng = np.random.default_rng(77)
    walk = np.cumsum(rng.standard_normal((80, most)) * 0.3, axis=1)
    truth = (-5 + walk + 0.5 * rng.standard_normal((80, most))).astype(np.float32)
    pos = np.sort(rng.integers(0, most, size=most))
    gen = (truth[:, pos] + 0.5 * rng.standard_normal((80, most))).astype(np.float32)
    basis = evaluation.cepstral_basis(80, 13, gpu)
    cost, steps, _ = _run(_pack([gen], [truth], gpu), basis)
    want_cost, want_steps, _, slots = ref.align([gen], [truth], basis.cpu().numpy())
    rel = abs(cost[0] - want_cost[0]) / want_cost[0]
    print(f"\n[dtw {most} x {most}] cost {cost[0]:.6f} vs {want_cost[0]:.6f}, rel {rel:.3e} (bound {17 * U:.3e}); steps {steps[0]} vs {want_steps[0]}, "
          f"margin {slots[0]['margin']:.3e}, E {slots[0]['E']:.3e}")
    assert rel <= 17 * U and most <= steps[0] <= 2 * most - 1
    if slots[0]["margin"] > 8 * slots[0]["E"]:
        assert steps[0] == want_steps[0]
