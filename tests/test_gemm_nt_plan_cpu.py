"""Host-side checks behind tests/test_gemm_nt_exact_hip.py (no GPU): the dispatcher of csrc/gemm_nt.hip restated in
tests/gemm_nt_plan.py agrees with the library's host-only entry points; the GPU case list reaches every path a plain GEMM can take;
every exact case keeps its partial sums inside fp32's integers; and the float64 expectations are not degenerate -- a kernel that
dropped, repeated or displaced a piece would fail the equality, and the normal-input bound rejects a missing k column."""
import pytest
import torch

import gemm_nt_plan as P


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from reformer_tts_amd import _lib
    return _lib.load()


def _large_shapes():
    s = {mn for c in P.CASES.values() for mn in c["shapes"]} | {(m, n) for _, m, n, *_ in P.NORMAL}
    s |= {(m, n) for g in P.GROUPS.values() for m, n, _, _ in g}
    return s | {(12288, 512), (12288, 1024), (12288, 2048), (16384, 2048), (16384, 512), (49152, 256), (3072, 2048)}


def test_restated_tile_pick_agrees_with_the_library(lib):
    """rtts_gemm_nt_partial_rows = (M / BM) WM of the picked tile (or -1) and rtts_gemm_nt_gate_words = tiles x 64 WM x 2 (0 for
    256 x 256 or no tile) launch nothing; both must equal the restatement on a grid of small shapes and on every large shape used."""
    shapes = [(m, n) for m in range(32, 1025, 32) for n in range(32, 513, 32)] + sorted(_large_shapes())
    bad, seen = [], set()
    for m, n in shapes:
        got = (lib.rtts_gemm_nt_partial_rows(m, n), lib.rtts_gemm_nt_gate_words(m, n))
        want = (P.partial_rows(m, n), P.gate_words(m, n))
        seen.add(P.gn_pick(m, n))
        if got != want:
            bad.append(((m, n), got, want))
    print(f"\n[gemm_nt plan] {len(shapes)} shapes, picks seen {sorted(seen)}")
    assert not bad, bad[:10]
    assert seen == {-1, 0, 1, 2, 3, 4}


def test_case_list_reaches_every_plain_path():
    """The set of path tags a plain GEMM can take is enumerated from the dispatcher's structure; the GPU case list must reach all
    of them and nothing outside the enumeration (a new ring depth, form or tile shows up here as an unknown tag)."""
    reach, cases = P.reachable_plain_tags(), P.all_case_tags()
    print(f"\n[gemm_nt plan] {len(reach)} reachable path tags, {len(P.CASE_PARAMS)} GPU cases")
    assert not reach - set(cases), sorted(reach - set(cases))
    assert not set(cases) - reach, sorted(set(cases) - reach)
    # what the issue names for each path is what the restated dispatcher sends it down
    for name, c in P.CASES.items():
        for (m, n) in c["shapes"]:
            for nk in c["nks"]:
                tag = P.nt_plan(m, n, 64 * nk, True, "5" if "delta" in c else "0")
                want_nst = 4 if "delta" in c else c["nst"]
                assert tag.startswith(f"{c['tile'][0]}x{c['tile'][1]}<") and f" NST{want_nst} form0 " in tag, (name, m, n, nk, tag)
    assert "<4,1>" in P.nt_plan(512, 128, 64, True, "5") and "<4,1>" in P.nt_plan(384, 256, 64, True, "5")
    for mn in ((192, 128), (576, 256)):
        assert P.nt_plan(*mn, 64, True, "5").startswith("192x128<4,2> NST4"), mn
    tiles = {(96, 64): (1, "96x64"), (192, 128): (4, "96x64"), (288, 64): (3, "96x64"), (1536, 768): (192, "96x64"),
             (128, 64): (1, "128x64"), (384, 256): (12, "128x64"), (2048, 768): (192, "128x64"), (8192, 2048): (256, "256x256"),
             (3072, 1536): (192, "192x128"), (6144, 2048): (512, "192x128"), (6144, 4096): (1024, "192x128"), (4096, 1536): (192, "256x128")}
    for (m, n), (cnt, tile) in tiles.items():
        bm, bn, _ = P.CAND[P.gn_pick(m, n)]
        assert (f"{bm}x{bn}", (m // bm) * (n // bn)) == (tile, cnt), (m, n)


def test_groups_reach_the_tiles_rings_and_spreads_asked_for():
    seen = set()
    for name, members in P.GROUPS.items():
        for kn in (False, True):
            tag, tile_end = P.group_plan([(m, n, k, e, 0, n + 8) for m, n, k, e in members], kn)
            tile, nst, spread = P.GROUP_EXPECT[name]
            assert tag.startswith(tile + "<") and f" NST{nst} form1 " in tag and tag.endswith(f"spread{spread}"), (name, tag)
            seen.add((tile, nst, spread, len(members)))
            if spread:
                assert all(t % 8 == 0 for t in tile_end)
    assert {(t, n, s) for t, n, s, _ in seen} >= {("192x128", 4, 1), ("192x128", 2, 1), ("192x128", 2, 0), ("96x64", 4, 1), ("96x64", 4, 0),
                                                  ("128x64", 4, 1), ("128x64", 4, 0)}
    assert {c for *_, c in seen} >= {2, 3, 4}
    assert P.group_plan([(1536, 1536, 64, "0", 0, 1544)] * 2)[1] == [96, 192]
    assert all(m % 96 for g in ("128x64_spread", "128x64_nospread") for m, *_ in P.GROUPS[g])
    assert sorted(k for _, _, k, _ in P.GROUPS["four_mixed_k_and_epilogues"]) == [64, 192, 320, 576]


def test_store_mode_restated():
    assert [P.gn_store_mode(a, ld) for a, ld in ((0x1000, 520), (0x1008, 520), (0x1000, 516), (0x1004, 520))] == [2, 0, 0, 0]
    assert P.gn_store_mode(0x1000, 520, forced=1) == 1 and P.gn_store_mode(0x1008, 520, forced=1) == 0 and P.gn_store_mode(0x1000, 520, 0) == 0
    for name, off, pad, dbg in P.PLACEMENTS:
        assert str(P.gn_store_mode(0x1000 + off, 512 + pad, dbg - 10 if dbg >= 10 else -1)) == P.EXPECTED_STORE[name]


def test_every_exact_case_keeps_its_sums_exact_in_fp32():
    worst = dict(product=0, colsum=0, delta=0)
    ks = [(64 * nk, c["tile"]) for c in P.CASES.values() for nk in c["nks"]]
    for name, members in P.GROUPS.items():
        ks += [(k, (192, 128)) for _, _, k, _ in members]
    for k, tile in ks:
        for key, v in P.exactness(k, tile).items():
            worst[key] = max(worst[key], v)
            assert v < 2 ** 24, (key, k, tile, v)
    assert 16 * 576 + 64 < 2 ** 24 and 64 * 4 * 16 * 576 < 2 ** 24
    print(f"\n[gemm_nt plan] largest magnitudes: {worst} (2^24 = {2 ** 24})")


# ------------------------------------------------------------------------------------------ the expectations are not degenerate
def _smallest(recipe):
    m, n, k, t = 96, 64, 128, 24
    ops = (P.int_operands if recipe == "int" else P.normal_operands)(m, n, k, 11, "cpu")
    return ops, t, P.expectations(ops, t)


def _with(ops, **kw):
    return dict(ops, **kw)


@pytest.mark.parametrize("recipe", ["int", "normal"])
def test_expectations_change_under_each_kernel_mistake(recipe):
    """Plain CPU arithmetic: at the smallest shape (96 x 64, K = 128 = two stages) each float64 expectation changes when one K
    stage is dropped or counted twice, one 16-row fragment is displaced by 16 rows, the bias is omitted, or one element's gate
    flips -- so a kernel doing any of these fails the equality (integers) or, for the normal inputs, the elementwise bound."""
    ops, t, e = _smallest(recipe)
    a, w = ops["a"], ops["w"]

    def differs(x, y, bf16):
        if recipe == "int":
            return not torch.equal(x.to(torch.bfloat16) if bf16 else x, y.to(torch.bfloat16) if bf16 else y)
        scale = a.abs() @ w.abs().t() if x.shape == e["ref"].shape else torch.ones_like(x)
        return P.normal_ratio(x, y, scale, bf16) > 1.0
    a_drop = a.clone()
    a_drop[:, 64:] = 0
    a_twice = a.clone()
    a_twice[:, :64] *= 2
    a_disp = a.clone()
    a_disp[16:32], a_disp[32:48] = a[32:48], a[16:32]
    mistakes = {"stage dropped": _with(ops, a=a_drop), "stage twice": _with(ops, a=a_twice), "fragment displaced": _with(ops, a=a_disp)}
    for what, bad_ops in mistakes.items():
        b = P.expectations(bad_ops, t)
        for key, bf16 in (("ref", True), ("ref", False), ("bias", True), ("relu", True), ("gated_table", True), ("gated_h", True), ("acc", False)):
            assert differs(b[key], e[key], bf16), (what, key)
        if recipe == "int":
            for key in ("colsum_table", "colsum_h", "delta"):
                if (what, key) == ("fragment displaced", "colsum_h"):
                    continue            # rows and their own gates move together: the sum over rows cannot see it (C does)
                assert not torch.equal(b[key], e[key]), (what, key)
            assert not torch.equal(b["h_open"], e["h_open"]), what
    assert differs(e["ref"], e["bias"], True) and differs(e["ref"], e["bias"], False), "bias omitted"
    assert differs(torch.relu(e["ref"]), e["relu"], True), "bias omitted under the ReLU"
    if recipe == "int":
        idx = ops["gate_idx"].clone()
        i, j = [int(v) for v in (e["ref"] != 0).nonzero()[0]]
        idx[i, j] = 5 - idx[i, j]                      # the table is closed for 0..2 and open for 3..5
        flipped = P.expectations(_with(ops, gate_idx=idx), t)
        assert not torch.equal(flipped["gated_table"].to(torch.bfloat16), e["gated_table"].to(torch.bfloat16))
        assert not torch.equal(flipped["colsum_table"], e["colsum_table"])
        assert e["h_open"].any() and not e["h_open"].all() and P.gate_open(ops["gate_idx"]).any()
        # roundings and ties happen: some |result| > 256 is not a bf16 value
        big = P.expectations(P.int_operands(96, 64, 576, 3, "cpu"))["ref"]
        assert (big.to(torch.bfloat16).double() != big).any()


def test_normal_input_bound_rejects_one_missing_k_column():
    """At the deepest K of the normal-input passes (576) the elementwise criterion rejects the float64 reference with ONE k column
    removed, for a bf16 and for an fp32 output -- and accepts the reference rounded once to bf16 resp. to fp32."""
    k = 64 * max(nk for *_, nk in [(c[0], c[3]) for c in P.NORMAL])
    ops = P.normal_operands(96, 64, k, 5, "cpu")
    a, w = ops["a"], ops["w"]
    ref, scale = a @ w.t(), a.abs() @ w.abs().t()
    miss = ref - torch.outer(a[:, k - 1], w[:, k - 1])
    r16, r32 = P.normal_ratio(miss, ref, scale, True), P.normal_ratio(miss, ref, scale, False)
    ok16 = P.normal_ratio(ref.to(torch.bfloat16).double(), ref, scale, True)
    ok32 = P.normal_ratio(ref.float().double(), ref, scale, False)
    print(f"\n[gemm_nt plan] K = {k}: one k column missing scores {r16:.1f} (bf16) / {r32:.1f} (fp32) of the bound; "
          f"the rounded reference {ok16:.3f} / {ok32:.2e}")
    assert r16 > 1 and r32 > 1 and ok16 <= 1 and ok32 <= 1


def test_gate_table_is_what_it_says():
    vals = torch.tensor(P.GATE_TABLE_BITS, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    assert vals[0] == -2 and vals[4] == 1 and vals[5] == 3 and vals[1] == 0 and vals[2] == 0
    assert torch.signbit(vals[1]) and not torch.signbit(vals[2])
    assert vals[3].double().item() == 2.0 ** -133
    assert [bool(v > 0) for v in vals.double()] == P.GATE_TABLE_OPEN


def test_gate_word_decoding_inverts_the_documented_map():
    """decode_gate_words against a direct per-bit loop over the documented map, on a 2 x 2 grid of 96 x 64 tiles."""
    m, n = 192, 128
    bm, bn, wm = P.CAND[P.gn_pick(m, n)]
    assert (bm, bn) == (96, 64)
    g = torch.Generator().manual_seed(0)
    mask = torch.rand(m, n, generator=g) < 0.5
    tm, tn, wn = bm // wm // 16, bn // 2 // 16, 2
    words = torch.zeros(P.gate_words(m, n), dtype=torch.int64)
    for row in range(m):
        for col in range(n):
            if not mask[row, col]:
                continue
            tile_m, rm = divmod(row, bm)
            tile_n, rn = divmod(col, bn)
            wmi, rm = divmod(rm, bm // wm)
            wni, rn = divmod(rn, bn // wn)
            i, r = divmod(rm, 16)
            j, rn = divmod(rn, 16)
            gq, el = divmod(rn, 4)
            tid = 64 * (wmi * wn + wni) + 16 * gq + r
            words[(tile_m * (n // bn) + tile_n) * 64 * wm * wn + tid] |= 1 << ((i * tn + j) * 4 + el)
    got, clear = P.decode_gate_words(words, m, n)
    assert clear and torch.equal(got, mask)
    assert tm * tn * 4 == 24
