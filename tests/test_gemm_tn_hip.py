"""rtts_gemm_tn / rtts_gemm_tn_grouped (csrc/gemm_tn.hip) -- the split-K weight-gradient GEMM behind every weight gradient of
the stacks and the edges -- and engine.wgrad / flush_wgrad, on every path the host dispatcher can send a problem down:
the 128 x 128 tile kernel and the 256 x 256 ring kernel, unsplit and split (with a stage count split does not divide), runs
shorter than the ring depth, a workspace that runs short or is absent, strided operands, groups of 1 .. 16 problems, and the
groups the product itself launches.

Two references in every case, both in float64 on the same bf16 operands:
  * EXACT INTEGERS (the main check).  dY and X hold integers in [-4, 4], C0 integers in [-64, 64]: all exact in bf16 and fp32,
    every product |a b| <= 16 is exact, and every partial sum any summation order can form is an integer of magnitude
    <= 16 M + 64 < 2^24 (asserted per case; M up to ~1M would do, the largest case here is 49,216 rows), so fp32 represents it
    exactly.  The result is then independent of how the token range is split, staged, reduced or tiled, and every path must
    equal the float64 product BIT FOR BIT: a dropped, repeated or misplaced row, stage, slab or tile fails.
  * NORMAL INPUTS with an elementwise bound.  bf16 N(0, 1) operands (and a case whose token rows are scaled by 2^-6 / 1 / 2^6):
    max |got - ref| / (|dY|^T |X| + |C0|) <= 2^-16, far above fp32 summation noise (~2^-24 of that scale per addition) and
    far below one token row's share of it (checked: the criterion rejects the reference with one row's outer product removed).
Each run also checks that nothing outside C's (N, K) window -- its padding columns (ldc > K), guard bands before and after it,
the slab workspace beyond what the call was given -- changed (a NaN bit pattern there), and that two runs of a normal-input
group are bitwise equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -16
GUARD = 64                  # floats of guard band around C and after the slab workspace (keeps 16-byte alignment)
NAN_BITS = 0x7FC0DEAD       # a quiet NaN with a payload no kernel writes
BF16_NAN = float("nan")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ the dispatcher, restated
def tn_plan(shapes, ws_floats, small_tiles=False):
    """Restates the host logic of ``rtts_gemm_tn_grouped`` (csrc/gemm_tn.hip:446-513, from ``bool big = ...`` to the launches):
    256 x 256 tiles (the ring kernel) unless rtts_debug_set_gemm_tn_tiles(1) is in force (``small_tiles``), when every N and
    K % 256 == 0 and the group reaches 40 GFLOP; one split target ``want`` for the group (the smallest power of two with tiles x 2 want > 320 resp. 640); per
    problem split doubles up to ``want`` while split x 2 <= (M / 64) / 4, then halves while the slab workspace cannot hold it
    (``ws_floats`` None = slab_ws NULL).  ``shapes``: (M, N, K) per problem -> (kernel, [split per problem], slab floats used).
    If the dispatcher changes, test_case_list_covers_every_dispatch_path fails here instead of a path going untested."""
    big = not small_tiles and all(n % 256 == 0 and k % 256 == 0 for _, n, k in shapes)
    if sum(2 * m * n * k for m, n, k in shapes) < 40 * 10 ** 9:
        big = False
    bt = 256 if big else 128
    tiles = sum((n // bt) * (k // bt) for _, n, k in shapes)
    want = 1
    while tiles * want * 2 <= (320 if big else 640):
        want *= 2
    used, splits = 0, []
    for m, n, k in shapes:
        split = 1
        while split < want and split * 2 <= (m // 64) // 4:
            split *= 2
        while split > 1 and (ws_floats is None or used + n * k * split > ws_floats):
            split //= 2
        if split > 1:
            used += n * k * split
        splits.append(split)
    return ("ring" if big else "tile128"), splits, used


def P(m, n, k, acc=1, pa=0, pb=0, pc=0):
    """One problem: M x N x K, accumulate, and extra leading-dimension elements of dY / X / C (a padded operand is also a view
    that starts 16 bytes into its buffer)."""
    return (m, n, k, acc, pa, pb, pc)


FULL = "full"               # a workspace as large as every split of the group needs
_S = 512 * 512              # one slab of a 512 x 512 gradient
_WS_GROUP = [P(3072, 512, 512, 1), P(3072, 512, 512, 0), P(3072, 512, 512, 1)]            # 8 ways each with room for it
# a group the ring kernel takes (45 GFLOP, every N, K % 256 == 0) that also holds an M = 64 problem (two 32-row ring stages:
# fewer than the three the ring keeps in flight) and an M = 128 one (four stages: the counted waits 2, 2, 1, 0)
_RING_GROUP = [P(12288, 1024, 512, 1), P(12288, 2048, 512, 0), P(12288, 512, 512, 1), P(64, 256, 256, 1), P(128, 512, 256, 1)]
# (name, problems, workspace floats | FULL | None, rtts_debug_set_gemm_tn_tiles(1) in force)
CASES = [
    ("t128_split1", [P(256, 128, 128, 0)], FULL, False),
    ("t128_split16_rem11", [P(64 * 75, 128, 128, 1)], FULL, False),        # 75 stages over 16 runs: the first 11 one stage longer
    ("ring_split32_rem2", [P(49216, 1024, 512, 1)], FULL, False),          # 1538 ring stages over 32 runs
    ("ring_group_short_runs", _RING_GROUP, FULL, False),
    ("ring_group_on_t128", _RING_GROUP, FULL, True),
    ("ws_halves", _WS_GROUP, 5 * _S, False),                # splits 4, 1, 1
    ("ws_exact_boundary", _WS_GROUP, 6 * _S, False),        # 4, then 2 with slab_used + slab * 2 == ws, then 1
    ("ws_one_short", _WS_GROUP, 6 * _S - 4, False),         # 4, 1, 1
    ("ws_null", _WS_GROUP, None, False),                    # slab_ws = NULL: 1, 1, 1
    ("strided_t128", [P(1024, 256, 384, 1, 24, 8, 12), P(2048, 128, 256, 0, 8, 40, 4), P(4800, 384, 128, 1, 16, 16, 20)], FULL, False),
    ("strided_ring", [P(12288, 1024, 512, 1, 64, 8, 4), P(12288, 2048, 512, 0, 8, 24, 12), P(12288, 512, 512, 1, 16, 64, 8)], FULL, False),
    ("group2", [P(1024, 256, 128, 1), P(512, 128, 384, 0)], FULL, False),
    ("group7", [P(2048, 512, 512, 1), P(3072, 128, 256, 1), P(256, 256, 128, 0), P(1024, 384, 128, 1), P(64, 128, 128, 1),
                P(4800, 256, 256, 0), P(640, 128, 512, 1)], FULL, False),
    ("group16", [P(64 * (1 + (i * 37) % 48), 128 * (1 + i % 3), 128 * (1 + (i * 5) % 4), int(i % 3 != 0)) for i in range(16)], FULL, False),
]
_IDS = [c[0] for c in CASES]


def _plan(problems, ws, small):
    shapes = [(m, n, k) for m, n, k, *_ in problems]
    if ws == FULL:
        ws = tn_plan(shapes, 1 << 62, small)[2]
    kernel, splits, used = tn_plan(shapes, ws, small)
    return kernel, splits, used, ws


def case_paths(problems, ws, small):
    """The dispatch paths one case takes (by tn_plan)."""
    kernel, splits, used, ws_f = _plan(problems, ws, small)
    shapes = [(m, n, k) for m, n, k, *_ in problems]
    free = tn_plan(shapes, 1 << 62, small)[1]
    tags = {f"group of {len(problems)}"}
    for (m, *_), sp in zip(problems, splits):
        if kernel == "tile128":
            tags.add("tile128 split 1" if sp == 1 else "tile128 split >= 2")
            if sp > 1 and (m // 64) % sp:
                tags.add("tile128 stages % split != 0")
        elif kernel == "ring":
            tags.add("ring split 1" if sp == 1 else "ring split >= 2")
            if sp > 1 and (m // 32) % sp:
                tags.add("ring stages % split != 0")
            if (m // 32) // sp < 3:
                tags.add("ring run shorter than the ring depth")
    if small and tn_plan(shapes, ws_f, False)[0] == "ring":
        tags.add("ring-sized group on the 128-tile kernel")
    if 1 in splits and max(splits) > 1:
        tags.add("split and unsplit problems in one group")
    if ws is None and max(free) > 1:
        tags.add("slab_ws NULL")
    elif ws != FULL and any(s < f for s, f in zip(splits, free)):
        tags.add("workspace short: split halved")
        if used == ws:
            tags.add("workspace exact boundary")
    if any(pa or pb or pc for *_, pa, pb, pc in problems) and len({p[3] for p in problems}) == 2:
        tags.add("strided operands, accumulate on and off in one group")
    return tags


REQUIRED = {
    "tile128 split 1", "tile128 split >= 2", "tile128 stages % split != 0", "ring split 1", "ring split >= 2", "ring stages % split != 0",
    "ring run shorter than the ring depth", "ring-sized group on the 128-tile kernel", "split and unsplit problems in one group",
    "workspace short: split halved", "workspace exact boundary", "slab_ws NULL", "strided operands, accumulate on and off in one group",
    "group of 1", "group of 2", "group of 7", "group of 16",
}


def test_case_list_covers_every_dispatch_path(gpu):
    """Every row of the dispatch table is reached by some case (judged by tn_plan, the dispatcher restated); the product's own
    groups are replayed by test_product_groups_replayed_exactly."""
    seen = {}
    for name, problems, ws, small in CASES:
        for t in case_paths(problems, ws, small):
            seen.setdefault(t, []).append(name)
    for t in sorted(REQUIRED):
        print(f"\n  {t:55s} {', '.join(seen.get(t, ['-']))}", end="")
    print()
    assert REQUIRED <= set(seen), sorted(REQUIRED - set(seen))


# ------------------------------------------------------------------------------------------ operands and one launch
def _bf16_operand(m, cols, pad, vals, dev):
    """(m, cols) bf16 view with leading dimension cols + pad (NaN in the padding: a kernel that read it would spread NaN)."""
    if not pad:
        return vals.to(torch.bfloat16).contiguous()
    flat = torch.full((8 + m * (cols + pad),), BF16_NAN, dtype=torch.bfloat16, device=dev)
    v = flat[8:].view(m, cols + pad)[:, :cols]
    v.copy_(vals)
    return v


class _CBuf:
    """(n, k) fp32 window with leading dimension k + pad inside a buffer whose every other float holds NAN_BITS."""

    def __init__(self, n, k, pad, c0):
        self.ld = k + pad
        self.bits = torch.full((2 * GUARD + n * self.ld,), NAN_BITS, dtype=torch.int32, device=c0.device)
        self.c = self.bits.view(torch.float32)[GUARD:GUARD + n * self.ld].view(n, self.ld)[:, :k]
        self.c.copy_(c0)
        self.outside = torch.ones_like(self.bits, dtype=torch.bool)
        self.outside[GUARD:GUARD + n * self.ld].view(n, self.ld)[:, :k] = False

    def untouched(self):
        return bool((self.bits[self.outside] == NAN_BITS).all())


def _operands(problems, ints, seed, dev, row_scale=False):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for m, n, k, acc, pa, pb, pc in problems:
        if ints:
            a = torch.randint(-4, 5, (m, n), generator=g, device=dev).float()
            b = torch.randint(-4, 5, (m, k), generator=g, device=dev).float()
            c0 = torch.randint(-64, 65, (n, k), generator=g, device=dev).float()
        else:
            a = torch.randn(m, n, generator=g, device=dev)
            b = torch.randn(m, k, generator=g, device=dev)
            c0 = torch.randn(n, k, generator=g, device=dev)
            if row_scale:           # token rows at 2^-6, 1, 2^6 (exact in bf16), dY and X out of step
                r = torch.arange(m, device=dev)
                a = a * torch.pow(2.0, 6.0 * (r % 3 - 1).float())[:, None]
                b = b * torch.pow(2.0, 6.0 * ((r // 3) % 3 - 1).float())[:, None]
        out.append((_bf16_operand(m, n, pa, a, dev), _bf16_operand(m, k, pb, b, dev), c0, acc, pc))
    return out


def _launch(ops, ws, small=False):
    """One rtts_gemm_tn_grouped call over ``ops`` (``small``: under rtts_debug_set_gemm_tn_tiles(1), the library's pick again on
    the way out) -> (results as float64, C and workspace untouched outside the windows)."""
    from reformer_tts_amd import _lib
    dev = ops[0][0].device
    cbufs = [_CBuf(a.shape[1], b.shape[1], pc, c0) for a, b, c0, _, pc in ops]
    wsb = None
    if ws is not None:
        wsb = torch.full((ws + GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
    arr = (_lib.GemmTnProblem * len(ops))()
    for e, (a, b, _, acc, _), cb in zip(arr, ops, cbufs):
        e.a, e.lda, e.b, e.ldb, e.c, e.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), cb.c.data_ptr(), cb.ld
        e.M, e.N, e.K, e.accumulate = a.shape[0], a.shape[1], b.shape[1], acc
    _lib.call("rtts_debug_set_gemm_tn_tiles", int(small))
    try:
        _lib.call("rtts_gemm_tn_grouped", arr, len(ops), None if wsb is None else wsb.data_ptr(), 0 if ws is None else ws,
                  torch.cuda.current_stream().cuda_stream)
    finally:
        _lib.call("rtts_debug_set_gemm_tn_tiles", 0)
    torch.cuda.synchronize()
    clean = all(cb.untouched() for cb in cbufs) and (wsb is None or bool((wsb[ws:] == NAN_BITS).all()))
    return [cb.c.double() for cb in cbufs], clean


def _refs(ops):
    """float64 dY^T X (+ C0) and |dY|^T |X| (+ |C0|) per problem."""
    out = []
    for a, b, c0, acc, _ in ops:
        a64, b64 = a.double(), b.double()
        ref, scale = a64.t() @ b64, a64.abs().t() @ b64.abs()
        if acc:
            ref, scale = ref + c0.double(), scale + c0.double().abs()
        out.append((ref, scale))
    return out


def _ratio(got, ref, scale):
    return ((got - ref).abs() / scale).max().item()


def _run_case(problems, ws, small):
    kernel, splits, _, ws_f = _plan(problems, ws, small)
    return kernel, splits, ws_f


# ------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name,problems,ws,small", CASES, ids=_IDS)
def test_gemm_tn_exact_on_integers(gpu, name, problems, ws, small):
    """Bit-exact against the float64 product of integer operands (see the module docstring for why every path must be)."""
    for m, *_ in problems:
        assert m * 16 + 64 < 2 ** 24, "partial sums must stay exact in fp32"
    kernel, splits, ws_f = _run_case(problems, ws, small)
    ops = _operands(problems, True, 1, gpu)
    got, clean = _launch(ops, ws_f, small)
    bad = []
    for i, (g, (ref, _)) in enumerate(zip(got, _refs(ops))):
        if not torch.equal(g, ref):
            d = (g - ref).abs()
            nz = d.nonzero()
            bad.append(f"problem {i} {problems[i][:3]}: {nz.shape[0]} elements differ (max {d.max().item():g}; first at {nz[0].tolist()})")
    print(f"\n[gemm_tn {name}] {kernel}, splits {splits}, ws {ws_f}: "
          f"{'bit-exact' if not bad else 'MISMATCH'} on {len(problems)} integer problem(s); outside C untouched: {clean}")
    assert not bad, "; ".join(bad)
    assert clean, "the kernel wrote outside C's (N, K) window or beyond the slab workspace it was given"


@pytest.mark.parametrize("name,problems,ws,small", CASES, ids=_IDS)
def test_gemm_tn_float64_bound_and_determinism(gpu, name, problems, ws, small):
    """bf16 N(0,1) operands: max |got - ref| / (|dY|^T |X| + |C0|) <= 2^-16 per problem, two runs bitwise equal.  At the largest
    M of the case list the same criterion must reject the reference with one token row's outer product removed."""
    kernel, splits, ws_f = _run_case(problems, ws, small)
    ops = _operands(problems, False, 2, gpu)
    got1, clean1 = _launch(ops, ws_f, small)
    got2, clean2 = _launch(ops, ws_f, small)
    refs = _refs(ops)
    ratios = [_ratio(g, r, s) for g, (r, s) in zip(got1, refs)]
    print(f"\n[gemm_tn {name}] {kernel}, splits {splits}: max |err| / scale {max(ratios):.3e} (bound {BOUND:.3e} = 2^-16)")
    assert all(torch.equal(x, y) for x, y in zip(got1, got2)), "two runs of one group differ"
    assert clean1 and clean2
    assert max(ratios) <= BOUND, ratios
    m_max = max(p[0] for c in CASES for p in c[1])
    for i, (m, *_) in enumerate(problems):
        if m == m_max:          # the bound's sharpness, at the largest M used: no kernel involved
            a64, b64 = ops[i][0].double(), ops[i][1].double()
            ref, scale = refs[i]
            miss = ref - torch.outer(a64[m - 1], b64[m - 1])
            r_miss = _ratio(miss, ref, scale)
            print(f"  self-check at M = {m}: the reference without its last token row scores {r_miss:.3e} > {BOUND:.3e}")
            assert r_miss > BOUND, "the bound cannot see one missing token row at this M"


@pytest.mark.parametrize("name", ["t128_split16_rem11", "ring_group_short_runs"])
def test_gemm_tn_float64_bound_with_rows_scaled(gpu, name):
    """Token rows of dY and X scaled by 2^-6 / 1 / 2^6 (out of step): the elementwise bound holds where magnitudes mix."""
    _, problems, ws, small = next(c for c in CASES if c[0] == name)
    kernel, splits, ws_f = _run_case(problems, ws, small)
    ops = _operands(problems, False, 3, gpu, row_scale=True)
    got, clean = _launch(ops, ws_f, small)
    ratios = [_ratio(g, r, s) for g, (r, s) in zip(got, _refs(ops))]
    print(f"\n[gemm_tn {name}, rows scaled 2^+-6] {kernel}, splits {splits}: max |err| / scale {max(ratios):.3e} (bound {BOUND:.3e})")
    assert clean
    assert max(ratios) <= BOUND, ratios


# ------------------------------------------------------------------------------------------ the product's own groups
def _record_groups(monkeypatch, fn):
    """Run ``fn`` with _lib.call wrapped: -> every weight-gradient launch it made, as lists of (M, N, K, lda, ldb, ldc, accumulate)."""
    from reformer_tts_amd import _lib
    rec, orig = [], _lib.call

    def spy(name, *args):
        if name == "rtts_gemm_tn_grouped":
            rec.append([(p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.accumulate) for p in args[0][:args[1]]])
        elif name == "rtts_gemm_tn":
            a, lda, b, ldb, m, n, k, c, ldc, acc = args[:10]
            rec.append([(m, n, k, lda, ldb, ldc, acc)])
        return orig(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    try:
        fn()
    finally:
        monkeypatch.setattr(_lib, "call", orig)
    return rec


def _product_groups(gpu, monkeypatch):
    """The weight-gradient launches of one FusedStackFn backward of a decoder layer (B = 12, T = 1024 mel frames, 256 text
    positions as keys) and of an encoder block (B = 12, its 256 text positions) at the baseline widths: d = 512, 8 heads,
    buckets 128 / 64, 8 rounds, feed-forward 2048."""
    from reformer_tts_amd import engine
    from reformer_tts_amd.model.reformer import ReformerDec, ReformerEnc
    from oracle.model_ref import SMALL_LSH
    e, heads = 512, 8
    torch.manual_seed(5)
    lsh = dict(SMALL_LSH, implementation="hip", heads=heads, n_hashes=8)
    dec = ReformerDec(e, depth=1, ff_chunks=100, self_attn_kwargs=dict(lsh, bucket_size=128), ff_kwargs=dict(hidden=2048, dropout=0.0),
                      attn_kwargs=dict(num_heads=heads, dropout=0.0, bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None,
                                       vdim=None)).to(gpu).train()
    enc = ReformerEnc(e, depth=1, ff_chunks=100, attn_kwargs=dict(lsh, bucket_size=64), ff_kwargs=dict(hidden=2048, dropout=0.0)).to(gpu).train()
    groups = {}
    x = torch.randn(12, 1024, e, device=gpu, requires_grad=True)
    keys = torch.randn(12, 256, e, device=gpu, requires_grad=True)
    y, _ = dec(x, keys=keys, key_padding_mask=torch.zeros(12, 256, dtype=torch.bool, device=gpu), input_mask=None)
    assert dec.layers._program is not None, "the decoder layer did not take the explicit executor"

    def back_dec():
        y.sum().backward()
        engine.flush_wgrad()
    groups["decoder layer"] = _record_groups(monkeypatch, back_dec)
    xe = torch.randn(12, 256, e, device=gpu, requires_grad=True)
    ye = enc(xe)
    ye = ye[0] if isinstance(ye, tuple) else ye
    assert enc.layers._program is not None, "the encoder block did not take the explicit executor"

    def back_enc():
        ye.sum().backward()
        engine.flush_wgrad()
    groups["encoder block"] = _record_groups(monkeypatch, back_enc)
    torch.cuda.synchronize()
    return groups


def test_product_groups_replayed_exactly(gpu, monkeypatch):
    """The launches a decoder layer's and an encoder block's backward make, replayed with fresh integer operands of the same
    shapes and strides (slab workspace of the product's size): bit-exact, nothing outside C touched."""
    from reformer_tts_amd import engine
    groups = _product_groups(gpu, monkeypatch)
    n = 0
    for where, launches in groups.items():
        assert launches, f"{where}: no weight-gradient launch recorded"
        for j, launch in enumerate(launches):
            problems = [P(m, nn, k, acc, lda - nn, ldb - k, ldc - k) for m, nn, k, lda, ldb, ldc, acc in launch]
            for m, *_ in problems:
                assert m * 16 + 64 < 2 ** 24
            kernel, splits, _, _ = _plan(problems, engine._SLAB_FLOATS, False)
            ops = _operands(problems, True, 10 + j, gpu)
            got, clean = _launch(ops, engine._SLAB_FLOATS)
            exact = all(torch.equal(g, r) for g, (r, _) in zip(got, _refs(ops)))
            print(f"\n[gemm_tn {where} launch {j}] {kernel}, splits {splits}, problems (M, N, K, lda, ldb, ldc, acc) {launch}: "
                  f"{'bit-exact' if exact else 'MISMATCH'}, outside C untouched: {clean}")
            assert exact and clean, (where, j, launch)
            n += 1
    assert n >= 2


# ------------------------------------------------------------------------------------------ engine.wgrad / flush_wgrad
def _int_pair(m, n, k, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    dy = torch.randint(-4, 5, (m, n), generator=g, device=dev).to(torch.bfloat16)
    x = torch.randint(-4, 5, (m, k), generator=g, device=dev).to(torch.bfloat16)
    return dy, x, (dy.double().t() @ x.double())


def _grad_view(n, k, pad, seed, dev):
    """(n, k) fp32 gradient view with leading dimension k + pad, integers in [-64, 64]; -> (view, its initial value)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    buf = torch.randint(-64, 65, (n, k + pad), generator=g, device=dev).float()
    return buf[:, :k], buf[:, :k].double().clone()


def test_engine_wgrad_every_branch_exact(gpu):
    """engine.wgrad against the exact integer reference on each of its branches: the split-K kernel direct (accumulate=False),
    queued then flushed (accumulate=True under DEFER_WGRAD), the zero-padded K < 128 form (K = 80 mel channels over 4096
    rows), and the library GEMM for a shape that does not tile."""
    from reformer_tts_amd import engine
    assert engine.DEFER_WGRAD
    engine.flush_wgrad()
    for label, (m, n, k), acc in (("direct", (1024, 256, 384), False), ("deferred", (1024, 256, 384), True),
                                  ("K < 128 padded", (4096, 256, 80), False), ("K < 128 padded", (4096, 256, 80), True),
                                  ("library", (200, 96, 100), False), ("library", (200, 96, 100), True)):
        dy, x, prod = _int_pair(m, n, k, m + k + acc, gpu)
        gv, g0 = _grad_view(n, k, 12, n + k, gpu)
        engine.wgrad(gv, dy, x, accumulate=acc)
        queued = engine.pending_wgrads()
        engine.flush_wgrad()
        torch.cuda.synchronize()
        want = prod + g0 if acc else prod
        print(f"\n[engine.wgrad {label}, accumulate={acc}] {m} x {n} x {k}: queued {queued}, "
              f"{'bit-exact' if torch.equal(gv.double(), want) else 'MISMATCH'}")
        assert queued == (1 if label == "deferred" else 0)
        assert torch.equal(gv.double(), want), (label, acc, (gv.double() - want).abs().max().item())


def _count_grouped(monkeypatch):
    from reformer_tts_amd import _lib
    calls, orig = [], _lib.call

    def spy(name, *args):
        if name == "rtts_gemm_tn_grouped":
            calls.append(args[1])
        return orig(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    return calls


def test_flush_of_more_than_a_group_of_entries(gpu, monkeypatch):
    """20 queued weight gradients flush as two grouped launches (16 + 4) and each receives exactly its own product."""
    from reformer_tts_amd import engine
    engine.flush_wgrad()
    items = []
    for i in range(20):
        m, n, k = 64 * (4 + i % 5), 128 * (1 + i % 2), 128 * (1 + i % 3)
        dy, x, prod = _int_pair(m, n, k, 100 + i, gpu)
        gv, g0 = _grad_view(n, k, 4 * (i % 2), 200 + i, gpu)
        engine.wgrad(gv, dy, x)
        items.append((gv, g0 + prod))
    assert engine.pending_wgrads() == 20
    calls = _count_grouped(monkeypatch)
    engine.flush_wgrad()
    torch.cuda.synchronize()
    print(f"\n[flush of 20 entries] grouped launches of {calls} problems")
    assert calls == [16, 4]
    assert all(torch.equal(gv.double(), want) for gv, want in items)


def test_one_gradient_queued_twice_receives_both_contributions(gpu, monkeypatch):
    """A weight queued twice before a flush (a backward through two forwards of one model) must receive both products.  In one
    grouped launch the two problems' workgroups race on the same C (one contribution lost, varying run to run), so the flush
    starts a new launch at the second entry -- launch order stays the queue's order."""
    from reformer_tts_amd import engine
    engine.flush_wgrad()
    gv, g0 = _grad_view(512, 512, 0, 7, gpu)
    other, o0 = _grad_view(256, 512, 0, 8, gpu)
    dy1, x1, p1 = _int_pair(3072, 512, 512, 1, gpu)
    dy2, x2, p2 = _int_pair(3072, 512, 512, 2, gpu)
    dy3, x3, p3 = _int_pair(1024, 256, 512, 3, gpu)
    engine.wgrad(gv, dy1, x1)
    engine.wgrad(other, dy3, x3)
    engine.wgrad(gv, dy2, x2)
    calls = _count_grouped(monkeypatch)
    engine.flush_wgrad()
    torch.cuda.synchronize()
    ok = torch.equal(gv.double(), g0 + p1 + p2)
    lost = (gv.double() - (g0 + p1 + p2)).abs().max().item()
    print(f"\n[one gradient queued twice] grouped launches of {calls} problems; both contributions there: {ok} (max diff {lost:g})")
    assert ok
    assert torch.equal(other.double(), o0 + p3)


def test_other_deferred_gradients_queued_twice_receive_both_contributions(gpu):
    """The other deferred gradient work has the same hazard as the weight gradients: the column sums of a bias / LayerNorm
    gradient (engine.flush_colsum: one launch adds every queued partial buffer into its output) and the re-layout of a
    convolution's weight gradient (edges.flush_conv_dw: dw += its taps).  One output queued twice must receive both
    (integer values: exact)."""
    from reformer_tts_amd import edges, engine
    engine.flush_wgrad()
    g = torch.Generator(device=gpu).manual_seed(12)
    q = engine._queue()
    rows, d = engine._partial_rows(4096), 512
    out = torch.randint(-64, 65, (d,), generator=g, device=gpu).float()
    other = torch.randint(-64, 65, (d,), generator=g, device=gpu).float()
    want_out, want_other = out.double().clone(), other.double().clone()
    for tgt, want in ((out, want_out), (other, want_other), (out, want_out)):
        part = torch.randint(-64, 65, (rows * d,), generator=g, device=gpu).float()
        q.colsums.append((part, 0, rows, d, tgt, 0))
        want += part.view(rows, d).double().sum(0)
    engine.flush_colsum(q)
    co, ci, cp = 128, 80, 128
    dw = torch.randint(-64, 65, (co, ci, 5), generator=g, device=gpu).float()
    want_dw = dw.double().clone()
    for _ in range(2):
        dwp = torch.randint(-64, 65, (co, 5 * cp), generator=g, device=gpu).float()
        q.conv_items.append((dwp, co, ci, cp, dw))
        want_dw += dwp.double().view(co, 5, cp)[:, :, :ci].transpose(1, 2)
    edges.flush_conv_dw(q)
    torch.cuda.synchronize()
    res = (torch.equal(out.double(), want_out), torch.equal(other.double(), want_other), torch.equal(dw.double(), want_dw))
    print(f"\n[deferred column sums / conv dW queued twice] both contributions there: {res}")
    assert all(res)


def test_gemm_tn_grouped_refuses_overlapping_outputs(gpu):
    """rtts_gemm_tn_grouped refuses two problems that write a common element of C, and takes disjoint column blocks of one
    matrix (the five tap problems of a convolution's weight gradient) -- whose results are exact."""
    from reformer_tts_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    dy, x, prod = _int_pair(512, 128, 128, 4, gpu)
    c = torch.zeros(256, 640, device=gpu)

    def prob(e, cptr, ldc):
        e.a, e.lda, e.b, e.ldb, e.c, e.ldc = dy.data_ptr(), 128, x.data_ptr(), 128, cptr, ldc
        e.M, e.N, e.K, e.accumulate = 512, 128, 128, 1

    def group(*cs):
        arr = (_lib.GemmTnProblem * len(cs))()
        for e, (ptr, ldc) in zip(arr, cs):
            prob(e, ptr, ldc)
        return arr
    base = c.data_ptr()
    refused = [
        ((base, 640), (base, 640)),                               # the same C
        ((base, 640), (base + 4 * 64, 640)),                      # columns 64.. of the same rows
        ((base, 640), (base + 4 * 640 * 100, 640)),               # rows 100.. of the same columns
        ((base, 640), (base + 4 * 512, 640), (base + 4 * 96, 640)),
        ((base, 640), (base + 4 * 600, 640)),                      # starts at column 600, its rows wrap into the first's columns
        ((base, 640), (base + 4 * 128, 256)),                      # different ldc, spans interleave
    ]
    for cs in refused:
        with pytest.raises(_lib.RttsError, match="overlapping"):
            _lib.call("rtts_gemm_tn_grouped", group(*cs), len(cs), None, 0, s)
    # five disjoint 128-column blocks of one (128, 640) matrix
    cs = [(base + 4 * 128 * t, 640) for t in range(5)]
    _lib.call("rtts_gemm_tn_grouped", group(*cs), 5, None, 0, s)
    # below them, a window whose rows wrap round the row end (columns 600.. and 0..87 of the next row) beside one it misses
    c2 = torch.zeros(256, 640, device=gpu)
    wrap = 127 * 640 + 600
    _lib.call("rtts_gemm_tn_grouped", group((c2.data_ptr(), 640), (c2.data_ptr() + 4 * wrap, 640)), 2, None, 0, s)
    torch.cuda.synchronize()
    for t in range(5):
        assert torch.equal(c[:128, 128 * t:128 * (t + 1)].double(), prod)
    assert not c[128:].any()
    assert torch.equal(c2[:128, :128].double(), prod)
    assert torch.equal(torch.as_strided(c2, (128, 128), (640, 1), wrap).double(), prod)
    inside = torch.zeros(256, 640, dtype=torch.bool, device=gpu)
    inside[:128, :128] = True
    torch.as_strided(inside, (128, 128), (640, 1), wrap).fill_(True)
    assert not c2[~inside].any()
