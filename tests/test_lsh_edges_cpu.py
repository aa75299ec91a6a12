"""CPU half of the LSH attention edge tests: the constructed inputs of tests/lsh_edges_ref.py are PROVEN to reach the branches they
are listed for (branch census), the vectorised float64 oracle is held to the brute-force definition on exactly those inputs, and
the float64 rounding model is held to the oracle's autograd with its roundings switched off.  No GPU."""
import functools

import pytest
import torch

import lsh_edges_ref as R
from oracle import lsh_ref

HD = R.H * R.DH
PAIRS = [(c, k) for c in R.CASES for k in R.DATA_KINDS]
PAIR_IDS = [f"{R.case_id(c)}-{k}" for c, k in PAIRS]


@functools.lru_cache(maxsize=None)
def _census(case, kind):
    return R.census_of(case, kind)


def _line(z):
    return ", ".join(f"{k} {z[k]}" for k in R.CENSUS_KEYS)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_constructed_permutations_are_valid(case):
    """Every round of every (batch, head) row is a permutation of 0..T-1 (what the kernels index with), the four rows differ, and
    the families have the shape they are named for."""
    st = R.make_st(case.family, case.t, case.bs, case.rounds, R.CASES.index(case))
    R.check_st(st, case.t)
    assert st.shape == (R.B * R.H, case.rounds, case.t)
    for i in range(st.shape[0]):
        for j in range(i):
            assert not torch.equal(st[i], st[j]), "two (batch, head) rows share a permutation: a wrong row index would not show"
    bs = case.bs
    if case.family in ("ascending", "descending"):
        step = 1 if case.family == "ascending" else -1
        d = (st[:, :, 1:] - st[:, :, :-1])
        assert int((d != step).sum()) == st.shape[0] * case.rounds - case.rounds        # one seam per rotated row and round
    if case.family == "echo":
        for r in range(case.rounds):
            ends = st[:, r, -bs:].sort(dim=-1).values
            begins = st[:, (r + 1) % case.rounds, :bs].sort(dim=-1).values
            assert torch.equal(ends, begins)


def test_padding_mask_has_the_listed_lengths():
    for t, bs in ((256, 64), (512, 128)):
        m = R.make_mask(t, bs)
        assert m.sum(dim=1).tolist() == [t - t // 3, bs + 6]
        assert bool(m[:, 0].all()) and not bool(m[:, -1].any())


def test_ramp_logits_are_a_cosine_of_the_angle_difference():
    """ramp(A): q . k / |k| / 8 = A cos(pi (i - j) / T) up to the 2 % noise -- what makes the logits monotonic along a sorted chunk."""
    t = 256
    qk = R.heads_first(R.make_qkv("ramp", t)[..., :HD])[0]
    logits = (qk @ (qk / qk.norm(dim=-1, keepdim=True)).T) / 8.0
    i = torch.arange(t, dtype=torch.float64)
    want = R.RAMP_A * torch.cos(torch.pi * (i[:, None] - i[None, :]) / t)
    # noise: 0.02 * 8A per dimension on q and on k => sqrt(2) * 0.02 * A * ... ~ 2.3 nats rms on a logit of up to 80
    rms = float((logits - want).pow(2).mean().sqrt())
    print(f"\n[ramp({R.RAMP_A:.0f})] rms deviation of the logits from A cos: {rms:.2f} nats, range {float(logits.min()):.1f} .. {float(logits.max()):.1f}")
    assert rms < 4.0 and float(logits.max()) > 75.0


def test_census_matches_the_closed_form_of_an_ordered_causal_input():
    """ascending + causal, nothing padded: per round and row every own chunk has nt(nt-1)/2 dead tiles above the diagonal, as many
    live ones below it and nt mixed ones on it; every looked-back half is wholly live except the one at the seam, which is wholly
    dead (nt empty waves); position 0 sees only itself in every round; nothing wraps onto itself."""
    case = next(c for c in R.CASES if c.family == "ascending" and c.causal and not c.masked and c.t == 256)
    z = _census(case, "unit")
    rows, nb, nt = R.B * R.H * case.rounds, case.t // case.bs, case.bs // 32
    assert z["waves"] == rows * nb * nt * 2
    assert z["dead_tiles"] == rows * (nb * nt * (nt - 1) // 2 + nt * nt)
    assert z["live_tiles"] == rows * (nb * nt * (nt - 1) // 2 + (nb - 1) * nt * nt)
    assert z["mixed_tiles"] == rows * nb * nt
    assert z["empty_waves"] == rows * nt and z["per_round_empty"].tolist() == [R.B * R.H * nt] * case.rounds
    assert z["wrap_self_pairs"] == 0 and z["padded_chunks"] == 0
    assert z["self_only"] == rows and z["self_only_rows"].nonzero()[:, 1].tolist() == [0] * (R.B * R.H)
    assert z["self_count"][:, 0].tolist() == [case.rounds] * (R.B * R.H)


@pytest.mark.parametrize("case,kind", PAIRS, ids=PAIR_IDS)
def test_case_reaches_what_it_is_listed_for(case, kind):
    """Conditions on the INPUTS (tests/lsh_edges_ref.py::expectations): the GPU file runs exactly these (case, data) pairs."""
    z = _census(case, kind)
    print(f"\n[census {R.case_id(case)} {kind}] {_line(z)}")
    for name, holds in R.expectations(case, kind).items():
        assert holds(z), f"{R.case_id(case)} / {kind} does not reach: {name} ({_line(z)})"


def test_every_branch_is_reached_by_construction_and_unit_data_reaches_no_rescale():
    """Over the whole table: rescale after the first live tile, wholly dead tile, wholly live tile, empty key half, wrap-self,
    wholly padded chunk and self-only row are each reached by a case that is BUILT to reach it (not by the luck of a random
    round); unit-scale data -- all the existing suite feeds these kernels -- reaches no rescale at all."""
    by = {(c, k): _census(c, k) for c, k in PAIRS}
    built = {
        "rescales": [(c, k) for c, k in PAIRS if k == "ramp" and c.family in ("ascending", "descending") and not (c.family == "descending" and c.causal)],
        "dead_tiles": [(c, k) for c, k in PAIRS if c.family == "ascending" and c.causal],
        "live_tiles": [(c, k) for c, k in PAIRS if c.family == "ascending" and c.causal],
        "empty_waves": [(c, k) for c, k in PAIRS if c.family in ("ascending", "descending") and c.causal],
        "wrap_self_pairs": [(c, k) for c, k in PAIRS if c.family == "echo"],
        "padded_chunks": [(c, k) for c, k in PAIRS if c.masked and c.family != "random"],
        "self_only": [(c, k) for c, k in PAIRS if c.causal or c.masked],
    }
    for key, pairs in built.items():
        counts = [by[p][key] for p in pairs]
        print(f"\n[reached by construction] {key}: {len(pairs)} (case, data) pairs, counts {min(counts)} .. {max(counts)}")
        assert pairs and min(counts) > 0, key
    unit = [by[(c, "unit")]["rescales"] for c in R.CASES]
    assert unit == [0] * len(R.CASES), unit
    assert len(R.CASES) == 24 and all(c.rounds in (2, 3, 4) for c in R.CASES)
    assert {(c.t, c.bs) for c in R.CASES} == {(256, 64), (512, 128)}


@pytest.mark.parametrize("family,kind,causal,masked", [("descending", "ramp", True, False), ("echo", "unit", False, True)])
def test_vectorised_oracle_matches_the_brute_force_on_constructed_inputs(family, kind, causal, masked):
    """float64 lsh_attention_sorted against lsh_attention_bruteforce (explicit loops over rounds, queries and keys) on one
    (batch, head) row at T = 256, bs = 64, R = 2.  Both are float64 and differ only in summation order: 1e-9 of max|v|, on rows
    that see another token (lse_tot > -1e4).  Protects the new tests against an indexing slip in the vectorised oracle on exactly
    the inputs where they lean on it."""
    t, bs, rounds, row = 256, 64, 2, 3
    qkv = R.make_qkv(kind, t, seed=5)
    qk, v = R.heads_first(qkv[..., :HD])[row:row + 1], R.heads_first(qkv[..., HD:])[row:row + 1]
    st = R.make_st(family, t, bs, rounds, seed=5)[row:row + 1]
    mask = R.head_mask(R.make_mask(t, bs))[row:row + 1] if masked else None
    sticker, undo = R.flat_perm(st)
    out, _, lse = lsh_ref.lsh_attention_sorted(qk, v, sticker, undo, bs, rounds, causal, mask, return_parts=True)
    lse_tot = torch.logsumexp(lse, dim=1)
    out_bf, lse_bf = lsh_ref.lsh_attention_bruteforce(qk, v, sticker, bs, rounds, causal, mask)
    assert out.dtype == torch.float64 and out_bf.dtype == torch.float64
    normal = lse_bf > -1e4
    vmax = float(v.abs().max())
    e_out = float((out - out_bf)[normal].abs().max()) / vmax
    e_lse = float((lse_tot - lse_bf)[normal].abs().max())
    print(f"\n[oracle vs brute force {family} {kind} causal={causal} masked={masked}] out {e_out:.2e} of max|v| (tol 1e-9), lse_tot {e_lse:.2e} "
          f"(tol 1e-9), {int(normal.sum())} of {normal.numel()} rows compared")
    assert int(normal.sum()) > t // 8
    assert e_out <= 1e-9 and e_lse <= 1e-9


MODEL_CASES = [(R.CASES[0], "ramp"), (R.CASES[4], "ramp"), (R.CASES[8], "unit"), (R.CASES[9], "ramp"), (R.CASES[12], "unit"), (R.CASES[18], "ramp"),
               (R.CASES[21], "ramp")]


@pytest.mark.parametrize("case,kind", MODEL_CASES, ids=[f"{R.case_id(c)}-{k}" for c, k in MODEL_CASES])
def test_rounding_model_without_roundings_is_the_exact_function(case, kind):
    """The chunked float64 forward and backward of lsh_edges_ref.lsh_model with its roundings off against float64 autograd through
    the oracle: 1e-12 of max|ref| on dqk and dv, 1e-12 on lse; o and out to 1e-10 of max|v| (the oracle forms a self-only row's
    probabilities and round weights from logsumexp values near -5e4, where float64 resolves 7e-12; the model subtracts the maximum).  The model is then the oracle plus roundings,
    not a second opinion."""
    d = R.build(case, kind)
    qk, v, dout = R.heads_first(d["qkv"][..., :HD]), R.heads_first(d["qkv"][..., HD:]), R.heads_first(d["dout"])
    m = R.head_mask(d["mask"])
    out, o, lse, dqk, dv = R.exact_grads(qk, v, d["st"], case.bs, case.causal, m, dout)
    got = R.lsh_model(qk, v, d["st"], case.bs, case.causal, m, dout, rounding=False)
    vmax = float(v.abs().max())
    e = {"o": float((got["o"] - o).abs().max()) / vmax, "out": float((got["out"] - out).abs().max()) / vmax,
         "lse": float(((got["lse"] - lse).abs() / (1 + lse.abs())).max()),
         "dqk": R.grad_metrics(got["dqk"], dqk)[0], "dv": R.grad_metrics(got["dv"], dv)[0]}
    print(f"\n[model without roundings vs float64 autograd {R.case_id(case)} {kind}] " + ", ".join(f"{k} {x:.1e}" for k, x in e.items()) +
          " (tol 1e-12; o, out 1e-10)")
    assert e["dqk"] <= 1e-12 and e["dv"] <= 1e-12 and e["lse"] <= 1e-12 and e["o"] <= 1e-10 and e["out"] <= 1e-10, e
    # and the roundings do something: the model with them differs at the bf16 level
    rounded = R.lsh_model(qk, v, d["st"], case.bs, case.causal, m, dout, rounding=True)
    assert 1e-4 < R.grad_metrics(rounded["dqk"], dqk)[2] < 1e-1 and 1e-4 < R.grad_metrics(rounded["dv"], dv)[2] < 1e-1
