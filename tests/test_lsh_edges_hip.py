"""GPU half of the LSH attention edge tests: the attention kernels on CONSTRUCTED permutations, padding masks and sharp logits
(tests/lsh_edges_ref.py; tests/test_lsh_edges_cpu.py proves on the CPU which branch every case reaches), and the three streaming
kernels of csrc/lsh_combine.hip on their own.  The oracle is oracle.lsh_ref.lsh_attention_sorted in float64 on the same bf16 inputs
and the same permutation; for the backward on sharp logits it is the float64 rounding model of lsh_edges_ref.lsh_model."""
import contextlib

import pytest
import torch

import lsh_edges_ref as R

pytestmark = pytest.mark.gpu

HD = R.H * R.DH
PAIRS = [(c, k) for c in R.CASES for k in R.DATA_KINDS]
PAIR_IDS = [f"{R.case_id(c)}-{k}" for c, k in PAIRS]
BWD_RUNS = (0, 1, 2, 4)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from reformer_tts_amd import ops as _ops
    return _ops


@pytest.fixture
def force_walk():
    """Force the run length of the walking kernels for the rest of the test (``_lib.forced_walk``); undone when the test ends."""
    from reformer_tts_amd import _lib
    stack = contextlib.ExitStack()

    def force(fwd=None, bwd=None):
        stack.enter_context(_lib.forced_walk(fwd, bwd))
    yield force
    stack.close()


# ------------------------------------------------------------------------------------------- shared runs (computed once, read only)
_FWD, _BWD, _CENSUS = {}, {}, {}


def _census(case, kind):
    if (case, kind) not in _CENSUS:
        _CENSUS[(case, kind)] = R.census_of(case, kind)
    return _CENSUS[(case, kind)]


def _forward(ops, force, case, kind):
    """Kernel forward of (case, kind) as the one-chunk kernel and as the walking kernel at the case's run length, and the float64
    oracle with its autograd.  Cached: several tests read it, none changes it."""
    key = (case, kind)
    if key in _FWD:
        return _FWD[key]
    from reformer_tts_amd import _lib
    d = R.build(case, kind)
    R.check_st(d["st"], case.t)                         # on the host, before the first launch
    assert d["qkv"].shape == (R.B, case.t, 2 * HD) and (d["mask"] is None or d["mask"].shape == (R.B, case.t))
    qkv_d = d["qkv"].cuda()
    qk_d, v_d = qkv_d[..., :HD], qkv_d[..., HD:]
    st_d = d["st"].cuda()
    mask_d = None if d["mask"] is None else d["mask"].cuda()
    runs = {}
    for run in (0, case.fwd_walk):
        force(fwd=run)
        assert _lib.load().rtts_lsh_attn_fwd_run_length(R.B, R.H, case.t, case.rounds, case.bs) == run
        o, lse = ops.lsh_attn_fwd(qk_d, v_d, st_d, R.H, case.bs, case.causal, mask_d)
        out, lse_tot = ops.lsh_combine_fwd(o, lse, R.B, R.H)
        torch.cuda.synchronize()
        runs[run] = dict(o=o, lse=lse, out=out, lse_tot=lse_tot)
    qk, v, dout = R.heads_first(d["qkv"][..., :HD]), R.heads_first(d["qkv"][..., HD:]), R.heads_first(d["dout"])
    m = R.head_mask(d["mask"])
    out_ref, o_ref, lse_ref, dqk_ref, dv_ref = R.exact_grads(qk, v, d["st"], case.bs, case.causal, m, dout)
    _FWD[key] = dict(d=d, qk_d=qk_d, v_d=v_d, st_d=st_d, mask_d=mask_d, runs=runs, qk=qk, v=v, dout=dout, m=m, out_ref=out_ref,
                     o_ref=o_ref, lse_ref=lse_ref, dqk_ref=dqk_ref, dv_ref=dv_ref)
    return _FWD[key]


def _backward(ops, force, case, kind):
    """Kernel backward of (case, kind) at the run lengths 0 (one-chunk kernel), 1, 2 and 4, from the one-chunk forward's out and
    lse_tot -> {run: (dqk, dv) (BH, T, dh) float64 on the CPU}."""
    key = (case, kind)
    if key in _BWD:
        return _BWD[key]
    from reformer_tts_amd import _lib
    f = _forward(ops, force, case, kind)
    fw = f["runs"][0]
    dout_d = f["d"]["dout"].cuda()
    res = {}
    for run in BWD_RUNS:
        force(bwd=run)
        assert _lib.load().rtts_lsh_attn_bwd_run_length(R.B, R.H, case.t, case.rounds, case.bs) == run
        dqk, dv = ops.lsh_attn_bwd(f["qk_d"], f["v_d"], f["st_d"], fw["out"], dout_d, fw["lse_tot"], R.H, case.bs, case.causal, f["mask_d"])
        torch.cuda.synchronize()
        res[run] = (R.heads_first(dqk.cpu()), R.heads_first(dv.cpu()))
    _BWD[key] = res
    return res


# ------------------------------------------------------------------------------------------------------------ 3a / 3b: forward
@pytest.mark.parametrize("case,kind", PAIRS, ids=PAIR_IDS)
def test_forward_vs_float64(ops, force_walk, case, kind):
    """Bounds of test_lsh_hip.py::test_attention_forward_vs_oracle, unchanged: lse rtol = atol = 1e-3; o and out max error <= 1.2e-2
    of max|v|, mean <= 8e-4 on rows with lse_tot > -1e4.  They hold at ANY logit scale: one bf16 rounding of each probability is 2^-9
    relative, summed against |v|; one bf16 rounding of o and one of out are 2^-9 each -- together <= ~2^-8 max|v| = 3.9e-3, plus fp32
    logit noise (~1e-5 log2 units at logits of 80 nats).  ``ramp`` data drives the lazy running maximum through its rescale (census:
    rescale events in a quarter to two thirds of the live waves; 0 at unit scale): a wrong alpha, a missed shift of the tile's
    logits or a misfiring `fresh` test shows here."""
    f = _forward(ops, force_walk, case, kind)
    vmax = f["v"].abs().max().item()
    lse_tot_ref = torch.logsumexp(f["lse_ref"], dim=1)
    normal = lse_tot_ref > -1e4
    for run, k in f["runs"].items():
        o, lse = k["o"].double().cpu(), k["lse"].double().cpu()
        out, lse_tot = R.heads_first(k["out"].cpu()), k["lse_tot"].double().cpu()
        e_lse = ((lse - f["lse_ref"]).abs() / (1 + f["lse_ref"].abs())).max().item()
        e_o = (o - f["o_ref"]).abs().max().item() / vmax
        e_out = (out[normal] - f["out_ref"][normal]).abs().max().item() / vmax
        e_mean = (out[normal] - f["out_ref"][normal]).abs().mean().item() / vmax
        print(f"\n[lsh edges forward {R.case_id(case)} {kind} run {run}] / max|v|: o max {e_o:.2e}, out max {e_out:.2e} mean {e_mean:.2e}; "
              f"lse max {e_lse:.2e} of 1+|lse|, lse range {float(f['lse_ref'][f['lse_ref'] > -1e4].min()):.1f} .. {float(f['lse_ref'].max()):.1f} "
              f"(tol 1.2e-2, 1.2e-2, 8e-4, 1e-3)")
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
        torch.testing.assert_close(lse, f["lse_ref"], rtol=1e-3, atol=1e-3)
        assert e_o <= 1.2e-2 and e_out <= 1.2e-2 and e_mean <= 8e-4, (e_o, e_out, e_mean)
        torch.testing.assert_close(lse_tot, lse_tot_ref, rtol=1e-3, atol=1e-3)


# ------------------------------------------------------------------------------------------------------------ 3c: bit identity
@pytest.mark.parametrize("case,kind", PAIRS, ids=PAIR_IDS)
def test_walking_forward_is_bit_identical_to_the_one_chunk_forward(ops, force_walk, case, kind):
    """The walking forward (runs of 2 or 4) skips tiles that are wholly dead and drops the masks on tiles that are wholly live, and
    claims bit-identical results: shown here on tiles that are dead / live BY CONSTRUCTION (ascending / descending + causal,
    wholly padded chunks), on empty key halves and on rescaling waves, not only on what a hash sort happens to produce."""
    f = _forward(ops, force_walk, case, kind)
    a, b = f["runs"][0], f["runs"][case.fwd_walk]
    z = _census(case, kind)
    print(f"\n[lsh edges walking forward {R.case_id(case)} {kind}] run {case.fwd_walk} vs the one-chunk kernel; the inputs hold {z['dead_tiles']} dead, "
          f"{z['live_tiles']} live, {z['mixed_tiles']} mixed tiles, {z['empty_waves']} empty waves, {z['rescales']} rescales")
    assert torch.equal(a["o"], b["o"]), "o differs from the one-chunk kernel"
    assert torch.equal(a["lse"], b["lse"]), "lse differs from the one-chunk kernel"
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["lse_tot"], b["lse_tot"])


# ------------------------------------------------------------------------------------------------------------ 3d: self-only rows
SELF_PAIRS = [(c, k) for c, k in PAIRS if c.causal or c.masked]


@pytest.mark.parametrize("case,kind", SELF_PAIRS, ids=[f"{R.case_id(c)}-{k}" for c, k in SELF_PAIRS])
def test_rows_that_see_only_themselves(ops, force_walk, case, kind):
    """Position 0 under causal and every padded token (the rows come from the census): the only probability is exp2(0) = 1 and the
    dead keys give exact zeros, so o = v[self] exactly in every round and the combine gives v[self] back: |out - v| <= 2^-8 |v|
    element-wise (one bf16 ulp; the sibling test allows 1e-1).  lse_tot = -5e4 + ln n within 8e-3 (two steps of fp32's grid at 5e4),
    n = how often the row meets itself over all rounds: n = R, except under ``echo`` for a padded token that sits in both chunks of
    a round boundary, or where a random round repeats one there (both copies carry the self constant: that round's lse is
    -5e4 + ln 2)."""
    f = _forward(ops, force_walk, case, kind)
    z = _census(case, kind)
    rows = z["self_only_rows"]
    n_self = z["self_count"][rows].double()
    assert int(rows.sum()) > 0
    if case.family in ("ascending", "descending"):      # (a random round may repeat a token across a round boundary by chance)
        assert bool((n_self == case.rounds).all())
    want_lse = R.SELF_LOGIT + torch.log(n_self)
    v_rows = f["v"][rows]
    for run, k in f["runs"].items():
        out = R.heads_first(k["out"].cpu())[rows]
        o = k["o"].double().cpu().transpose(0, 1)[:, rows]                      # (R, n, dh)
        lse_tot = k["lse_tot"].double().cpu()[rows]
        e_out = ((out - v_rows).abs() / v_rows.abs().clamp_min(1e-30)).max().item()
        e_lse = (lse_tot - want_lse).abs().max().item()
        exact, exact_o = bool(torch.equal(out, v_rows)), bool((o == v_rows.unsqueeze(0)).all())
        print(f"\n[lsh edges self-only rows {R.case_id(case)} {kind} run {run}] {int(rows.sum())} rows, self count {int(n_self.min())} .. {int(n_self.max())}: "
              f"max |out - v| / |v| {e_out:.2e} (tol 2^-8 = 3.9e-3), max |lse_tot - (-5e4 + ln n)| {e_lse:.2e} (tol 8e-3); "
              f"out == v bit for bit: {exact}; o == v in every round: {exact_o}")
        assert bool(((out - v_rows).abs() <= 2.0 ** -8 * v_rows.abs()).all())
        assert e_lse <= 8e-3


# ------------------------------------------------------------------------------------------------------------ 3e: backward, unit
def _grad_report(tag, got, ref):
    mx, mean, l2 = R.grad_metrics(got, ref)
    return (mx, mean, l2), f"{tag} max {mx:.2e} mean {mean:.2e} rel-L2 {l2:.2e}"


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_backward_vs_float64_autograd_unit(ops, force_walk, case):
    """Bounds of test_lsh_hip.py::test_attention_backward_vs_oracle_autograd, unchanged (of max|ref|: max 1.5e-2, mean 1e-3; rel-L2
    1e-2), at run lengths 0 and 4, plus two exact consequences for padded tokens, which no query sees and which see only
    themselves: dqk[pad] == 0 exactly, and |dv[pad] - dout[pad]| <= R * 2^-8 |dout| (R partial rows of dout / R, each rounded once
    to bf16, plus the final rounding)."""
    f = _forward(ops, force_walk, case, "unit")
    g = _backward(ops, force_walk, case, "unit")
    for run in (0, 4):
        dqk, dv = g[run]
        msgs = []
        for got, ref, name in ((dv, f["dv_ref"], "dv"), (dqk, f["dqk_ref"], "dqk")):
            (mx, mean, l2), msg = _grad_report(name, got, ref)
            msgs.append(msg)
        print(f"\n[lsh edges backward {R.case_id(case)} unit run {run}] errors / max|ref|: " + "; ".join(msgs) + " (tol max 1.5e-2, mean 1e-3, rel-L2 1e-2)")
        for got, ref, name in ((dv, f["dv_ref"], "dv"), (dqk, f["dqk_ref"], "dqk")):
            mx, mean, l2 = R.grad_metrics(got, ref)
            assert mx <= 1.5e-2 and mean <= 1e-3 and l2 <= 1e-2, (name, run, mx, mean, l2)
        if case.masked:
            pad = ~f["m"]
            dout_p, dv_p = f["dout"][pad], dv[pad]
            e_dv = ((dv_p - dout_p).abs() / dout_p.abs().clamp_min(1e-30)).max().item()
            print(f"[lsh edges backward {R.case_id(case)} unit run {run}] {int(pad.sum())} padded rows: max|dqk| {float(dqk[pad].abs().max()):.1e} (must be 0), "
                  f"max |dv - dout| / |dout| {e_dv:.2e} (tol R 2^-8 = {case.rounds * 2.0 ** -8:.2e})")
            assert bool((dqk[pad] == 0).all())
            assert bool(((dv_p - dout_p).abs() <= case.rounds * 2.0 ** -8 * dout_p.abs()).all())


# ------------------------------------------------------------------------------------------------------------ 3f: backward, sharp logits
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_backward_on_sharp_logits_vs_rounding_model(ops, force_walk, case):
    """ramp(80): dS = P' (dP - delta) cancels where P' is nearly one-hot, so the kernel's error at sharp logits has no one-line bound;
    it is measured against a reference instead.  E_model = (float64 model of the kernels' arithmetic with a bf16 rounding where the
    kernels round: lsh_edges_ref.lsh_model) - (exact float64 gradient), in the three metrics of the unit-data test; the kernel must
    stay within 4 x E_model per metric -- the margin this project gives a rounding model over accumulation order and the hardware
    exp2 / rsq (test_sw_likelihood_hip.py, test_prenet_rounding_hip.py).  E_model is computed here, never from the kernel's output;
    the CPU file holds the model with its roundings off to the exact gradient at 1e-12."""
    f = _forward(ops, force_walk, case, "ramp")
    g = _backward(ops, force_walk, case, "ramp")
    model = R.lsh_model(f["qk"], f["v"], f["d"]["st"], case.bs, case.causal, f["m"], f["dout"], rounding=True)
    bad = []
    for name, ref in (("dqk", f["dqk_ref"]), ("dv", f["dv_ref"])):
        e_model = R.grad_metrics(model[name], ref)
        for run in (0, 4):
            got = g[run][0 if name == "dqk" else 1]
            assert bool(torch.isfinite(got).all())
            e_k = R.grad_metrics(got, ref)
            ratios = [a / b for a, b in zip(e_k, e_model)]
            print(f"\n[lsh edges backward sharp {R.case_id(case)} {name} run {run}] kernel max {e_k[0]:.2e} mean {e_k[1]:.2e} rel-L2 {e_k[2]:.2e} | "
                  f"E_model {e_model[0]:.2e} {e_model[1]:.2e} {e_model[2]:.2e} | ratio {ratios[0]:.2f} {ratios[1]:.2f} {ratios[2]:.2f} (tol 4)")
            if max(ratios) > 4.0:
                bad.append((name, run, e_k, e_model))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ 3g: walking backward
def _walk_diff(g):
    worst = 0.0
    for run, (dqk, dv) in g.items():
        for got, ref in ((dqk, g[0][0]), (dv, g[0][1])):
            worst = max(worst, float((got - ref).abs().max()) / float(ref.abs().max()))
    return worst


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_walking_backward_vs_the_one_chunk_backward(ops, force_walk, case):
    """Bound and reasoning of test_lsh_hip.py::test_walking_backward_matches_the_one_chunk_kernel on the constructed cases (unit
    data, as there): at run length 1 every chunk is both ends of its run (two partial rows per key, like the one-chunk kernel): dV
    bit-identical; other run lengths differ by the bf16 roundings of their partial rows: 1.2e-2 of max|ref|."""
    g = _backward(ops, force_walk, case, "unit")
    assert torch.equal(g[1][1], g[0][1]), "dV at run length 1 differs from the one-chunk kernel"
    worst = _walk_diff(g)
    print(f"\n[lsh edges walking backward {R.case_id(case)} unit] run lengths {sorted(g)}: max |diff| / max|ref| vs the one-chunk kernel {worst:.2e} (tol 1.2e-2)")
    assert worst <= 1.2e-2


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_walking_backward_vs_the_one_chunk_backward_on_sharp_logits(ops, force_walk, case):
    """ramp(80).  dV at run length 1 is bit-identical, as at unit scale.  For the other run lengths the 1.2e-2 of max|ref| of the
    unit-data test has no derivation here: it takes a partial row to be no larger than the gradient, and at sharp logits the
    contributions to a key's row (dQ and dK of its own chunk, dK from the chunk that looks back at it, per round) cancel -- measured
    1.2e-2 ... 2.9e-2 of max|ref| between the two forms on the random and echo cases, while each form is within 1.25 x E_model of the
    exact gradient (test_backward_on_sharp_logits_vs_rounding_model).  What IS derivable holds element by element, with u = 2^-8 the
    largest relative error of one bf16 rounding and A = sum over rounds of |dQ| + |dK as own key| + |dK as looked-back key| (for dv:
    |dV as own key| + |dV as looked-back key|) from the float64 model:
      * every form rounds each partial row, or the on-chip sum of some of them, once (|a + b| <= |a| + |b|) and the result once more:
        each form is within u (A + |result|) of the unrounded sum, two forms within 2^-7 (A + |result|) of each other -- the dv bound;
      * dQ is parked as bf16 before dK joins it, and the two forms accumulate it in another order: where it rounds the other way it
        moves by one bf16 step, <= 2^-7 |dQ| <= 2^-7 A -- the dqk bound is 2^-7 (2 A + |result|)."""
    f = _forward(ops, force_walk, case, "ramp")
    g = _backward(ops, force_walk, case, "ramp")
    assert torch.equal(g[1][1], g[0][1]), "dV at run length 1 differs from the one-chunk kernel"
    model = R.lsh_model(f["qk"], f["v"], f["d"]["st"], case.bs, case.causal, f["m"], f["dout"], rounding=True)
    worst = {"dqk": 0.0, "dv": 0.0}
    for run, (dqk, dv) in g.items():
        for name, got, ref, tol in (("dqk", dqk, g[0][0], 2.0 ** -7 * (2 * model["dqk_mag"] + g[0][0].abs())),
                                    ("dv", dv, g[0][1], 2.0 ** -7 * (model["dv_mag"] + g[0][1].abs()))):
            ratio = ((got - ref).abs() / tol.clamp_min(1e-300)).max().item()
            worst[name] = max(worst[name], ratio)
    print(f"\n[lsh edges walking backward {R.case_id(case)} ramp] run lengths {sorted(g)}: max |diff| / max|ref| vs the one-chunk kernel {_walk_diff(g):.2e} "
          f"(the unit-data 1.2e-2 has no derivation here); element-wise |diff| / bound: dqk {worst['dqk']:.2f}, dv {worst['dv']:.2f} (tol 1)")
    assert worst["dqk"] <= 1.0 and worst["dv"] <= 1.0, worst


# ====================================================================================================================
# 4. the three streaming kernels of csrc/lsh_combine.hip, called directly
# ====================================================================================================================
STREAM_SHAPES = [(1, 2, 40), (2, 3, 256)]      # (B, H, T): 80 rows = 640 threads, the last block partial; and one larger
SENTINEL = -777.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _wide(b, t, h, extra, dtype=torch.bfloat16):
    """A (B, T, H*64 + extra) buffer of sentinels and its (B, T, H*64) view: the kernels write rows with ld > H * 64."""
    buf = torch.full((b, t, h * R.DH + extra), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[..., :h * R.DH]


def _surplus_untouched(buf, h):
    return bool((buf[..., h * R.DH:] == torch.tensor(SENTINEL, dtype=buf.dtype)).all())


def _guarded(n, dtype=torch.float32, guard=16):
    """n elements followed by ``guard`` sentinels (a partial last block must not write past its rows)."""
    return torch.full((n + guard,), SENTINEL, dtype=dtype, device="cuda")


def _combine(o, lse, b, h, extra=24):
    from reformer_tts_amd import _lib
    bh, rounds, t, dh = o.shape
    buf, out = _wide(b, t, h, extra)
    lse_tot = _guarded(bh * t)
    _lib.call("rtts_lsh_combine_fwd", o.data_ptr(), lse.data_ptr(), b, h, t, dh, rounds, out.data_ptr(), out.stride(1),
              lse_tot.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _surplus_untouched(buf, h), "rtts_lsh_combine_fwd wrote beyond H * 64 columns"
    assert bool((lse_tot[bh * t:] == SENTINEL).all()), "rtts_lsh_combine_fwd wrote beyond lse_tot"
    return out.clone(), lse_tot[:bh * t].view(bh, t).clone()


def _bf16_ulp(x):
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


COMBINE_CASES = [(STREAM_SHAPES[0], r, p) for r in (1, 3, 8, 16) for p in ("normal", "ahead", "all_self", "some_self")] + \
                [(STREAM_SHAPES[1], 8, p) for p in ("normal", "ahead", "all_self", "some_self")]


@pytest.mark.parametrize("shape,rounds,pattern", COMBINE_CASES, ids=[f"B{s[0]}H{s[1]}T{s[2]}-R{r}-{p}" for s, r, p in COMBINE_CASES])
def test_combine_fwd_vs_float64(ops, shape, rounds, pattern):
    """rtts_lsh_combine_fwd against float64 from the same bf16 o and fp32 lse.  out: |err| <= 2^-8 |ref| + 1e-5 max|o| (one bf16
    rounding plus the fast exp's relative error, below 1e-5 for weights that matter); lse_tot: |err| <= 1e-5 + 2^-22 |ref|.
    lse patterns: 5 + randn; one round ahead of the others by 200 (every other weight underflows); every round exactly -5e4 (rows
    that see only themselves: out = the bf16 mean of the rounds' o within one ulp); some rounds -5e4 and the rest normal (those
    rounds have weight EXACTLY 0: out and lse_tot are bit-identical to a call given only the normal rounds)."""
    b, h, t = shape
    bh = b * h
    g = torch.Generator().manual_seed(100 * rounds + t)
    o = torch.randn(bh, rounds, t, R.DH, generator=g).bfloat16()
    lse = 5.0 + torch.randn(bh, rounds, t, generator=g)
    self_rounds = torch.zeros(rounds, dtype=torch.bool)
    if pattern == "ahead":
        lead = torch.randint(0, rounds, (bh, 1, t), generator=g)
        lse = lse + 200.0 * (torch.arange(rounds).view(1, rounds, 1) == lead)
    elif pattern == "all_self":
        lse = torch.full_like(lse, R.SELF_LOGIT)
    elif pattern == "some_self":
        self_rounds = torch.arange(rounds) % 3 == 1
        lse[:, self_rounds] = R.SELF_LOGIT
    out, lse_tot = _combine(o.cuda(), lse.cuda(), b, h)
    out = R.heads_first(out.cpu(), h)
    lse_tot = lse_tot.double().cpu()
    o64, l64 = o.double(), lse.double()
    mx = l64.max(dim=1, keepdim=True).values
    w = torch.exp(l64 - mx)
    ref = (w.unsqueeze(-1) * o64).sum(dim=1) / w.sum(dim=1).unsqueeze(-1)
    ref_lse = (mx + torch.log(w.sum(dim=1, keepdim=True))).squeeze(1)
    omax = float(o64.abs().max())
    err, tol = (out - ref).abs(), 2.0 ** -8 * ref.abs() + 1e-5 * omax
    err_l, tol_l = (lse_tot - ref_lse).abs(), 1e-5 + 2.0 ** -22 * ref_lse.abs()
    print(f"\n[combine_fwd B={b} H={h} T={t} R={rounds} {pattern}] out: max err {float(err.max()):.2e}, max err / tol {float((err / tol).max()):.2f}; "
          f"lse_tot: max err {float(err_l.max()):.2e}, max err / tol {float((err_l / tol_l).max()):.2f} (tol: 2^-8 |ref| + 1e-5 max|o|; 1e-5 + 2^-22 |ref|)")
    assert bool((err <= tol).all()) and bool((err_l <= tol_l).all())
    if pattern == "all_self":
        mean = R._bf16(o64.mean(dim=1))
        ulps = ((out - mean).abs() / _bf16_ulp(mean)).max().item()
        print(f"[combine_fwd all rounds at -5e4] out vs the bf16 mean of the rounds' o: {ulps:.2f} ulp (tol 1)")
        assert ulps <= 1.0
    if pattern == "some_self" and bool(self_rounds.any()):
        keep = ~self_rounds
        out2, lse_tot2 = _combine(o[:, keep].contiguous().cuda(), lse[:, keep].contiguous().cuda(), b, h)
        assert torch.equal(R.heads_first(out2.cpu(), h), out), "a round at -5e4 beside normal rounds did not have weight exactly 0"
        assert torch.equal(lse_tot2.double().cpu(), lse_tot)


def test_combine_fwd_refuses_more_than_16_rounds(ops):
    from reformer_tts_amd import _lib
    b, h, t, rounds = 1, 2, 40, 17
    o = torch.zeros(b * h, rounds, t, R.DH, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(b * h, rounds, t, device="cuda")
    out = torch.zeros(b, t, h * R.DH, dtype=torch.bfloat16, device="cuda")
    lse_tot = torch.zeros(b * h, t, device="cuda")
    with pytest.raises(_lib.RttsError, match="n_hashes <= 16"):
        _lib.call("rtts_lsh_combine_fwd", o.data_ptr(), lse.data_ptr(), b, h, t, R.DH, rounds, out.data_ptr(), h * R.DH, lse_tot.data_ptr(), _stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=[f"B{s[0]}H{s[1]}T{s[2]}" for s in STREAM_SHAPES])
def test_bwd_delta_vs_float64(ops, shape):
    """rtts_lsh_bwd_delta = rowsum(out * dout) per head against float64 from the bf16 inputs, out and dout with DIFFERENT row
    strides: |err| <= 2^-18 * sum |out| |dout| per row (the products are exact in fp32; 64 fp32 additions)."""
    from reformer_tts_amd import _lib
    b, h, t = shape
    g = torch.Generator().manual_seed(7 + t)
    out_c, dout_c = torch.randn(b, t, h * R.DH, generator=g).bfloat16(), torch.randn(b, t, h * R.DH, generator=g).bfloat16()
    buf_o, out = _wide(b, t, h, 8)
    buf_d, dout = _wide(b, t, h, 40)
    out.copy_(out_c)
    dout.copy_(dout_c)
    delta = _guarded(b * h * t)
    assert out.stride(1) != dout.stride(1)
    _lib.call("rtts_lsh_bwd_delta", out.data_ptr(), out.stride(1), dout.data_ptr(), dout.stride(1), b, h, t, R.DH, delta.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool((delta[b * h * t:] == SENTINEL).all()), "rtts_lsh_bwd_delta wrote beyond its rows"
    assert _surplus_untouched(buf_o, h) and _surplus_untouched(buf_d, h)
    a64, d64 = R.heads_first(out_c, h), R.heads_first(dout_c, h)
    ref = (a64 * d64).sum(dim=-1)
    tol = 2.0 ** -18 * (a64.abs() * d64.abs()).sum(dim=-1)
    err = (delta[:b * h * t].view(b * h, t).double().cpu() - ref).abs()
    print(f"\n[bwd_delta B={b} H={h} T={t}] max err {float(err.max()):.2e}, max err / tol {float((err / tol).max()):.3f} (tol 2^-18 sum|out||dout|)")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("flagged", [False, True], ids=["both-slots", "row-flags"])
@pytest.mark.parametrize("shape,rounds", [(STREAM_SHAPES[0], 3), (STREAM_SHAPES[0], 8), (STREAM_SHAPES[1], 4)],
                         ids=["B1H2T40-R3", "B1H2T40-R8", "B2H3T256-R4"])
def test_bwd_reduce_vs_float64(ops, shape, rounds, flagged):
    """rtts_lsh_bwd_reduce against the float64 sum over rounds and slots: |err| <= 2^-8 |ref| + 2^-19 * sum |partials| (one bf16
    rounding of the result, fp32 additions).  ``row_flags`` = None: both slots everywhere.  With a flag table (about a tenth of the
    rows set) slot 1 of every unflagged row holds NaN: the kernel must not read it -- the result is finite, within the same bound
    of the sum that leaves those slots out, and bit-identical to a call without flags whose unflagged slot-1 rows are zero."""
    from reformer_tts_amd import _lib
    b, h, t = shape
    bh = b * h
    slots = _lib.load().rtts_lsh_bwd_qk_slots()
    assert slots >= 2
    g = torch.Generator().manual_seed(31 * rounds + t)
    dqk_part = torch.randn(slots, bh, rounds, t, R.DH, generator=g).bfloat16()
    dv_part = torch.randn(2, bh, rounds, t, R.DH, generator=g).bfloat16()
    flags = (torch.rand(bh, rounds, t, generator=g) < 0.1) if flagged else torch.ones(bh, rounds, t, dtype=torch.bool)
    assert not flagged or 0.03 < float(flags.float().mean()) < 0.25

    def run(dqk_p, dv_p, fl):
        buf_q, dqk = _wide(b, t, h, 16)
        buf_v, dv = _wide(b, t, h, 16)
        dqk_d, dv_d = dqk_p.cuda(), dv_p.cuda()
        fl_d = None if fl is None else fl.to(torch.uint8).cuda()
        _lib.call("rtts_lsh_bwd_reduce", dqk_d.data_ptr(), dv_d.data_ptr(), b, h, t, R.DH, rounds, dqk.data_ptr(), dv.data_ptr(), dqk.stride(1),
                  None if fl_d is None else fl_d.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert _surplus_untouched(buf_q, h) and _surplus_untouched(buf_v, h), "rtts_lsh_bwd_reduce wrote beyond H * 64 columns"
        return R.heads_first(dqk.cpu(), h), R.heads_first(dv.cpu(), h)

    zeroed_q, zeroed_v = dqk_part.clone(), dv_part.clone()
    zeroed_q[1:][:, ~flags] = 0
    zeroed_v[1][~flags] = 0
    if flagged:
        poison_q, poison_v = dqk_part.clone(), dv_part.clone()
        poison_q[1:][:, ~flags] = float("nan")
        poison_v[1][~flags] = float("nan")
        dqk, dv = run(poison_q, poison_v, flags)
        assert bool(torch.isfinite(dqk).all()) and bool(torch.isfinite(dv).all()), "slot 1 of an unflagged row was read"
        dqk0, dv0 = run(zeroed_q, zeroed_v, None)
        assert torch.equal(dqk, dqk0) and torch.equal(dv, dv0)
    else:
        dqk, dv = run(dqk_part, dv_part, None)
    for name, got, part in (("dqk", dqk, zeroed_q), ("dv", dv, zeroed_v)):
        p64 = part.double()
        ref, mag = p64.sum(dim=(0, 2)), p64.abs().sum(dim=(0, 2))
        err, tol = (got - ref).abs(), 2.0 ** -8 * ref.abs() + 2.0 ** -19 * mag
        print(f"\n[bwd_reduce B={b} H={h} T={t} R={rounds} flags={flagged}] {name}: max err {float(err.max()):.2e}, max err / tol {float((err / tol).max()):.2f} "
              f"(tol 2^-8 |ref| + 2^-19 sum|partials|)")
        assert bool((err <= tol).all()), name
