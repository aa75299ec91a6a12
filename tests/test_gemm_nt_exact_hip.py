"""rtts_gemm_nt / rtts_gemm_nt_gated / rtts_gemm_nt_grouped (csrc/gemm_nt.hip) -- the MFMA GEMM behind every Linear, projection and
1 x 1 convolution -- EXACTLY, on every tile, ring depth, launch form, epilogue and store form the host dispatcher can send a plain
problem down (tests/gemm_nt_plan.py restates the dispatcher and holds the case list; tests/test_gemm_nt_plan_cpu.py checks on the CPU
that the list reaches every path and that the expectations below are not degenerate).  Everything goes through the C ABI.

EXACT INTEGERS (the main check).  A and W hold integers in [-4, 4] (bf16), bias and C0 integers in [-64, 64] (fp32), `out` of
epilogue 5 integers in [-4, 4], the gate activation values from {-2, -0.0, +0.0, the smallest bf16 subnormal, 1, 3}.  Every product and
every partial sum in any order is an integer below 2^24 (asserted per case), so the fp32 accumulators are exact whatever the stage
order, ring depth or tile, and against float64 on the same operands
  * fp32 outputs (epilogue 4, +- bias, +- accumulate) are equal BIT FOR BIT;
  * bf16 outputs equal ref.to(bfloat16) bit for bit -- one round-to-nearest-even of a known integer (results above 256 round, and tie);
  * the gate words epilogue 2 writes reproduce bf16(relu(ref + bias)) != 0 through the lane -> element map, the input gradient gated
    by the words equals the one gated by the activation and both equal ref * (h > 0);
  * the partial column-sum rows (pre-filled with NaN) are all written, nothing behind them is, and their float64 sum is the column
    sum of the UNROUNDED gated product;
  * epilogue 5: dout is bit-equal to the plain [K][N] product and delta to sum_64(out * bf16(dout)).
K = 64 nk with nk in {1, NST - 1, NST, NST + 1, 2 NST + 1}: below, at and above the ring depth of each path.
BUFFERS.  Every operand and output is a window in a larger buffer (guard bands, lda = K + 8, ldw = K + 24 resp. N + 24, ldg = N + 4,
ld_aux = N + 12, NaN in every padding element); outputs are pre-filled with a NaN payload no kernel writes and everything outside
the window must be unchanged after each call.  Each call runs in three placements of C -- 16-byte aligned with ldc = N + 8 (store
form 2), the same entered 8 bytes later (form 0), ldc = N + 4 (form 0) -- and with forms 1 and 2 forced: bit-equal inside the window.
GROUPS (n = 2 .. 4, both layouts): every member exact as above and bit-equal to its single launch.
NORMAL INPUTS, one pass per tile at the path's deepest K: |got - ref| <= 2^-8 |ref| + 2^-16 |A| |W|^T elementwise (bf16; the second
term alone for fp32) -- fractional bits, which the integers cannot exercise.

The reference's gated product SELECTS (gate open ? product : +0.0), as the kernel does: product * mask would hold -0.0 under a closed
gate and a negative product -- an artefact of the multiplication, and the comparison here is of bits.

PATH TAGS COVERED (format: gemm_nt_plan's docstring).  All 156 tags of gemm_nt_plan.reachable_plain_tags() -- the list is
``sorted(gemm_nt_plan.all_case_tags())`` -- that is, for each layout and each of its epilogues (NT: 0 1 2 2w 4 4b 4a; KN: 0 3 3w 4 4b
4a; no words on 256 x 256), with every bf16 epilogue in the store forms st0, st1 and st2 and every fp32 one in stf:
  256x256<4,2> NST2 form0        192x128<4,2> NST4 form0        192x128<4,2> NST2 form0 (512 and 1024 tiles)
  256x128<4,2> NST3 form0        96x64<2,2> NST4 form0          128x64<2,2> NST4 form0
  192x128<4,2> NST4 form0 KN epi5 (the large grid and the small-grid branch)       128x64<4,1> NST4 form0 KN epi5
and the 18 group tags (form1, epi6, both layouts): 192x128 NST4 spread1 / NST2 spread1 / NST2 spread0 / NST4 spread0, 96x64 spread1 /
spread0 (twice: three and four members), 128x64 spread1 / spread0.
MEASURED on an MI355X (written down after the run, not targets):
  cases: 41 (path, nk) cases (18,704 checks between them while the three 1024-tile cases also ran the persistent launch forms
  that are gone since; those cases now run once), 18 group cases, 1 refusal case, 7 normal-input cases: 67 tests;
  wall time of this file: 4.0 s (pytest's total; the slowest test 0.6 s, the first one, which loads the kernels);
  normal-input pass, worst |err| / bound over the bf16 epilogues (and over the fp32 ones) per tile:
    256x256 0.983 (0.009)   192x128 NST4 0.979 (0.008)   192x128 NST2 0.985 (0.009)   256x128 0.982 (0.008)   96x64 0.979 (0.008)
    128x64 0.979 (0.009)    128x64<4,1> epilogue 5: dout 0.959, delta 0.003
  (a correctly rounded bf16 result sits at up to 1.0 of its bound by construction: half an ulp at the bottom of a binade);
  three in-bounds breaks of a scratch copy of the kernel, each run once: the prologue waiting for NST - 1 younger stages whatever nk
  (19 tests fail, every path at nk < NST among them), `nh` for `nh - 4` in the 16-byte store address (66 fail), the fragment's first row
  for the row in epilogue 5's batch index (exactly the 10 delta cases fail)."""

import pytest
import torch

import gemm_nt_plan as P

pytestmark = pytest.mark.gpu

GUARD = 64                        # elements of guard band on either side of every window (a multiple of 8: windows stay 16-byte aligned)
NAN16 = 0x7FAD                    # bf16 NaN payloads no kernel writes (as int16), 0x7FC0DEAD its fp32 companion
NAN32 = 0x7FC0DEAD
NANW = 0x7FF8DEADBEEF0BAD         # gate words: a word left unwritten keeps this pattern and fails the comparison with the expected mask


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------ windows in guarded buffers
class _Win:
    """(rows, cols) window with leading dimension ``ld`` that starts ``GUARD`` elements + ``byte_off`` bytes into a flat buffer
    whose every other element holds a NaN pattern.  ``data``: initial contents (inputs; None: an output, NaN all over)."""
    PAT = {torch.bfloat16: (torch.int16, NAN16), torch.float32: (torch.int32, NAN32), torch.int64: (torch.int64, NANW)}

    def __init__(self, dev, rows, cols, dtype, ld=None, byte_off=0, data=None):
        self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
        self.itype, self.pat = self.PAT[dtype]
        off = GUARD + byte_off // torch.empty((), dtype=dtype).element_size()
        self.off = off
        self.bits = torch.full((off + rows * self.ld + GUARD,), self.pat, dtype=self.itype, device=dev)
        self.view = torch.as_strided(self.bits.view(dtype), (rows, cols), (self.ld, 1), off)
        self.bview = torch.as_strided(self.bits, (rows, cols), (self.ld, 1), off)
        self.is_input = data is not None
        if data is not None:
            self.view.copy_(data)
            self.snapshot = self.bits.clone()

    @property
    def ptr(self):
        return self.view.data_ptr()

    def take(self):
        """An output after a call: -> (a copy of the window, was everything outside it left alone); the window is NaN again."""
        got = self.view.clone()
        self.bview.fill_(self.pat)
        return got, bool((self.bits == self.pat).all())

    def unchanged(self):
        return torch.equal(self.bits, self.snapshot)


def _same(x, y):
    """Bit equality (NaN patterns included; -0.0 differs from +0.0)."""
    it = _Win.PAT[x.dtype][0]
    return x.shape == y.shape and torch.equal(x.contiguous().view(it), y.contiguous().view(it))


def _where(got, want):
    """Where two windows differ: count, first index, the row / column pattern (which tile rows, which lanes)."""
    d = (got.double() != want.double()) | (got.isnan() != want.isnan())
    nz = d.nonzero()
    if nz.numel() == 0:
        return "bit patterns differ in the sign of zero or a NaN payload only"
    rows, cols = nz[:, 0].unique(), nz[:, 1].unique()
    return (f"{nz.shape[0]} of {d.numel()} elements differ; first at {nz[0].tolist()}: got {got[tuple(nz[0])].item()} want {want[tuple(nz[0])].item()}; "
            f"{rows.numel()} rows [{rows.min().item()}..{rows.max().item()}], rows % 16 in {sorted(set((rows % 16).tolist()))[:16]}, "
            f"{cols.numel()} columns [{cols.min().item()}..{cols.max().item()}], columns % 16 in {sorted(set((cols % 16).tolist()))[:16]}")


class _Ops:
    """The operands of one (M, N, K) on the GPU, every one in a guarded window, with the float64 expectations."""

    def __init__(self, dev, m, n, k, seed, recipe="int", t=None):
        self.m, self.n, self.k, self.t = m, n, k, t
        ops = (P.int_operands if recipe == "int" else P.normal_operands)(m, n, k, seed, dev)
        self.e = P.expectations(ops, t)
        bf, f32 = torch.bfloat16, torch.float32
        self.a = _Win(dev, m, k, bf, k + 8, data=ops["a"])
        self.w = _Win(dev, n, k, bf, k + 24, data=ops["w"])
        self.wkn = _Win(dev, k, n, bf, n + 24, data=ops["w"].t())
        self.bias = _Win(dev, 1, n, f32, data=ops["bias"][None])
        self.c0 = ops["c0"].float()
        table = torch.tensor(P.GATE_TABLE_BITS, dtype=torch.int32, device=dev).to(torch.int16).view(bf)
        self.gate = _Win(dev, m, n, bf, n + 4, data=table[ops["gate_idx"]])
        self.h = _Win(dev, m, n, bf, n + 4, data=self.e["relu"].to(bf))
        self.out = _Win(dev, m, n, bf, n + 12, data=ops["out"]) if t is not None else None
        self.scale = ops["a"].abs() @ ops["w"].abs().t() if recipe != "int" else None
        self.abs_bias, self.abs_c0 = ops["bias"].abs(), ops["c0"].abs()
        self.inputs = [x for x in (self.a, self.w, self.wkn, self.bias, self.gate, self.h, self.out) if x is not None]

    def inputs_unchanged(self):
        return all(x.unchanged() for x in self.inputs)


class _Place:
    """One placement of C: outputs of either type for an (M, N) problem."""

    def __init__(self, dev, m, n, name, byte_off, pad):
        self.name = name
        self.c16 = _Win(dev, m, n, torch.bfloat16, n + pad, byte_off)
        self.c32 = _Win(dev, m, n, torch.float32, n + pad) if byte_off == 0 else None


# ------------------------------------------------------------------------------------------ launches
def _single(o, kn, epi, cwin, words=None, colsum=None, gate=None):
    """rtts_gemm_nt / rtts_gemm_nt_gated on the operands ``o``."""
    from reformer_tts_amd import _lib
    w = o.wkn if kn else o.w
    bias = o.bias.ptr if epi in ("1", "2", "2w", "4b") else None
    code = int(epi[0])
    if words is not None:
        _lib.call("rtts_gemm_nt_gated", o.a.ptr, o.a.ld, w.ptr, w.ld, int(kn), o.m, o.n, o.k, cwin.ptr, cwin.ld, bias, code, words.ptr,
                  None if colsum is None else colsum.ptr, _stream())
    else:
        _lib.call("rtts_gemm_nt", o.a.ptr, o.a.ld, w.ptr, w.ld, int(kn), o.m, o.n, o.k, cwin.ptr, cwin.ld, bias, code,
                  None if gate is None else gate.ptr, 0 if gate is None else gate.ld, None if colsum is None else colsum.ptr, _stream())


def _fill(e, o, kn, epi, cwin, delta=None):
    """One rtts_gemm_nt_problem from the operands ``o`` (epi: "0", "1", "4", "4b", "4a", "5")."""
    w = o.wkn if kn else o.w
    e.a, e.lda, e.w, e.ldw, e.c, e.ldc = o.a.ptr, o.a.ld, w.ptr, w.ld, cwin.ptr, cwin.ld
    e.bias = o.bias.ptr if epi in ("1", "4b") else None
    e.aux, e.ld_aux, e.aux_out = (o.out.ptr, o.out.ld, delta.ptr) if epi == "5" else (None, 0, None)
    e.M, e.N, e.K, e.epilogue, e.accumulate, e.reserved = o.m, o.n, o.k, int(epi[0]), int(epi == "4a"), 0
    e.T, e.H = (o.t, o.n // 64) if epi == "5" else (0, 0)


def _grouped(members, kn):
    """rtts_gemm_nt_grouped over ``members``: (operands, epi, C window, delta window or None) each."""
    from reformer_tts_amd import _lib
    arr = (_lib.GemmNtProblem * len(members))()
    for e, (o, epi, cwin, delta) in zip(arr, members):
        _fill(e, o, kn, epi, cwin, delta)
    _lib.call("rtts_gemm_nt_grouped", arr, len(members), int(kn), _stream())


class _Modes:
    """rtts_debug_set_gemm_mode (store forms 9..12) for the length of a block; the library's pick (9) again on the way out."""

    def __init__(self, *modes):
        self.modes = modes

    def __enter__(self):
        from reformer_tts_amd import _lib
        for m in self.modes:
            _lib.call("rtts_debug_set_gemm_mode", m)

    def __exit__(self, *exc):
        from reformer_tts_amd import _lib
        _lib.call("rtts_debug_set_gemm_mode", 9)
        return False


# ------------------------------------------------------------------------------------------ one shape through every epilogue
class _Check:
    """Collects failures with the path tag of the call that produced them."""

    def __init__(self, case):
        self.case, self.bad, self.n = case, [], 0

    def bits(self, tag, what, got, want):
        self.n += 1
        if not _same(got, want):
            self.bad.append(f"[{tag}] {what}: {_where(got, want)}")

    def true(self, tag, what, ok):
        self.n += 1
        if not ok:
            self.bad.append(f"[{tag}] {what}")

    def done(self):
        assert not self.bad, f"{self.case}: {len(self.bad)} of {self.n} checks failed:\n  " + "\n  ".join(self.bad[:12])


def _expected_bf16(o):
    bf, e = torch.bfloat16, o.e
    return {"0": e["ref"].to(bf), "1": e["bias"].to(bf), "2": e["relu"].to(bf), "2w": e["relu"].to(bf), "3": e["gated_table"].to(bf),
            "3h": e["gated_h"].to(bf), "3w": e["gated_h"].to(bf)}


def _run_plain(chk, dev, o):
    """Every epilogue of a plain problem in every placement of C.  -> number of launches."""
    from reformer_tts_amd import _lib
    m, n, k, e = o.m, o.n, o.k, o.e
    want16 = _expected_bf16(o)
    want32 = {"4": e["ref"].float(), "4b": e["bias"].float(), "4a": e["acc"].float()}
    nwords, rows = _lib.load().rtts_gemm_nt_gate_words(m, n), _lib.load().rtts_gemm_nt_partial_rows(m, n)
    assert nwords == P.gate_words(m, n) and rows == P.partial_rows(m, n) and rows > 0
    words = _Win(dev, 1, nwords, torch.int64) if nwords else None
    good_words = None
    colsum = _Win(dev, rows, n, torch.float32)
    first, launches = {}, 0
    for name, off, pad, dbg in P.PLACEMENTS:
        pl = _Place(dev, m, n, name, off, pad)
        forced = dbg - 10 if dbg >= 10 else -1
        with _Modes(dbg):
            def tag(kn, epi, win):
                t = P.nt_plan(m, n, k, kn, epi, win.ptr, win.ld, forced)
                if epi[0] != "4":
                    assert t.endswith("st" + P.EXPECTED_STORE[name]), (t, name)
                return f"{t} | {name}"

            def bf16_out(key, kn, epi, launch, want_key=None):
                nonlocal launches
                t = tag(kn, epi, pl.c16)
                launch()
                launches += 1
                got, clean = pl.c16.take()
                chk.true(t, "wrote outside C's window", clean)
                chk.bits(t, "C against float64", got, want16[want_key or epi])
                if key in first:
                    chk.bits(t, "C against the aligned placement", got, first[key])
                else:
                    first[key] = got
                return t

            def colsum_out(t, want):
                got, clean = colsum.take()
                chk.true(t, "wrote behind the partial column-sum rows", clean)
                chk.true(t, "a partial column-sum row was left unwritten", not bool(got.isnan().any()))
                chk.true(t, "float64 sum of the partial rows != column sums of the unrounded gated product", torch.equal(got.double().sum(0), want))

            # ---- rtts_gemm_nt / rtts_gemm_nt_gated
            for epi in ("0", "1", "2"):
                bf16_out(("nt", epi), False, epi, lambda: _single(o, False, epi, pl.c16))
            bf16_out(("kn", "0"), True, "0", lambda: _single(o, True, "0", pl.c16))
            t = bf16_out(("kn", "3"), True, "3", lambda: _single(o, True, "3", pl.c16, colsum=colsum, gate=o.gate))
            colsum_out(t, e["colsum_table"])
            t = bf16_out(("kn", "3h"), True, "3", lambda: _single(o, True, "3", pl.c16, colsum=colsum, gate=o.h), want_key="3h")
            colsum_out(t, e["colsum_h"])
            if words is not None:
                t = bf16_out(("nt", "2w"), False, "2w", lambda: _single(o, False, "2w", pl.c16, words=words))
                gw, clean = words.take()
                chk.true(t, "wrote outside the gate words", clean)
                mask, high_clear = P.decode_gate_words(gw.view(-1), m, n)
                chk.true(t, "gate words != (bf16(relu(ref + bias)) != 0) through the lane -> element map", torch.equal(mask, e["h_open"]))
                chk.true(t, "bits above the tile's outputs set in a gate word", high_clear)
                if good_words is None:
                    good_words = _Win(dev, 1, nwords, torch.int64, data=gw)
                    o.inputs.append(good_words)
                else:
                    chk.bits(t, "gate words against the aligned placement", gw, good_words.view)
                t = bf16_out(("kn", "3w"), True, "3w", lambda: _single(o, True, "3w", pl.c16, words=good_words, colsum=colsum))
                colsum_out(t, e["colsum_h"])
                chk.bits(t, "gated by the words against gated by the activation", first[("kn", "3w")], first[("kn", "3h")])
            # ---- rtts_gemm_nt_grouped, n = 1
            for epi in ("0", "1"):
                t = bf16_out(("nt", epi), False, epi, lambda: _grouped([(o, epi, pl.c16, None)], False))
            bf16_out(("kn", "0"), True, "0", lambda: _grouped([(o, "0", pl.c16, None)], True))
            if pl.c32 is not None:
                for kn, epi, how in ((False, "4", "s"), (False, "4b", "s"), (True, "4", "s"), (True, "4b", "s"), (False, "4", "g"), (True, "4", "g"),
                                     (False, "4a", "g"), (True, "4a", "g")):
                    t = tag(kn, epi, pl.c32)
                    if epi == "4a":
                        pl.c32.view.copy_(o.c0)
                    if how == "s":
                        _single(o, kn, epi, pl.c32)
                    else:
                        _grouped([(o, epi, pl.c32, None)], kn)
                    launches += 1
                    got, clean = pl.c32.take()
                    chk.true(t, "wrote outside C's window (fp32)", clean)
                    chk.bits(t, f"fp32 C against float64 ({'grouped n = 1' if how == 'g' else 'single'})", got, want32[epi])
        del pl
    chk.true("inputs", "an operand buffer changed", o.inputs_unchanged())
    return launches


def _run_delta(chk, dev, o):
    """Epilogue 5 in every placement of dout: dout bit-equal to the plain [K][N] product, delta to sum_64(out * bf16(dout))."""
    m, n, k, t, e = o.m, o.n, o.k, o.t, o.e
    delta = _Win(dev, (m // t) * (n // 64), t, torch.float32)
    want, want_delta = e["ref"].to(torch.bfloat16), e["delta"].float()
    assert torch.equal(want_delta.double(), e["delta"])
    for name, off, pad, dbg in P.PLACEMENTS:
        pl = _Place(dev, m, n, name, off, pad)
        forced = dbg - 10 if dbg >= 10 else -1
        with _Modes(dbg):
            tag = f"{P.nt_plan(m, n, k, True, '5', pl.c16.ptr, pl.c16.ld, forced)} T={t} | {name}"
            assert tag.split(" T=")[0].endswith("st" + P.EXPECTED_STORE[name])
            _single(o, True, "0", pl.c16)
            plain, clean = pl.c16.take()
            chk.true(tag, "the plain product wrote outside C's window", clean)
            _grouped([(o, "5", pl.c16, delta)], True)
            dout, clean = pl.c16.take()
            chk.true(tag, "wrote outside dout's window", clean)
            chk.bits(tag, "dout against float64", dout, want)
            chk.bits(tag, "dout against the plain [K][N] product", dout, plain)
            dl, clean = delta.take()
            chk.true(tag, "wrote outside delta", clean)
            chk.bits(tag, "delta against sum_64(out * bf16(dout))", dl, want_delta)
    chk.true("inputs", "an operand buffer changed", o.inputs_unchanged())


@pytest.mark.parametrize("name,nk", P.CASE_PARAMS, ids=P.CASE_IDS)
def test_gemm_nt_exact_on_integers(gpu, name, nk):
    """One path of the dispatcher at one depth against the ring: every shape of the path, every epilogue, every placement of C."""
    c, k = P.CASES[name], 64 * nk
    for key, v in P.exactness(k, c["tile"]).items():
        assert v < 2 ** 24, (key, v)
    chk, launches = _Check(f"{name}-nk{nk}"), 0
    for idx, (m, n) in enumerate(c["shapes"]):
        t = c["delta"][idx] if "delta" in c else None
        o = _Ops(gpu, m, n, k, 1000 * nk + idx, "int", t)
        if t is not None:
            _run_delta(chk, gpu, o)
        else:
            launches += _run_plain(chk, gpu, o)
        del o
    torch.cuda.synchronize()
    print(f"\n[gemm_nt exact {name} nk={nk}] {chk.n} checks, {len(chk.bad)} failed")
    chk.done()


# ------------------------------------------------------------------------------------------ groups
def _group_members(dev, members, seed):
    return [(_Ops(dev, m, n, k, seed + i, "int"), epi) for i, (m, n, k, epi) in enumerate(members)]


@pytest.mark.parametrize("kn", [False, True], ids=["NT", "KN"])
@pytest.mark.parametrize("name", list(P.GROUPS))
def test_gemm_nt_groups_exact_and_equal_to_single_launches(gpu, name, kn):
    """Each member of a grouped launch against float64, bit for bit, and against the same descriptor launched alone; the fp32 member
    that accumulates does so into a strided `into` holding integers."""
    members = _group_members(gpu, P.GROUPS[name], 77)
    chk = _Check(f"group {name} {'KN' if kn else 'NT'}")
    outs = []
    for o, epi in members:
        f32 = epi[0] == "4"
        outs.append(_Win(gpu, o.m, o.n, torch.float32 if f32 else torch.bfloat16, o.n + (12 if f32 else 8)))
        assert P.exactness(o.k, (192, 128))["product"] < 2 ** 24
    tag, tile_end = P.group_plan([(o.m, o.n, o.k, epi, w.ptr, w.ld) for (o, epi), w in zip(members, outs)], kn)
    tile, nst, spread = P.GROUP_EXPECT[name]
    assert tag.startswith(tile) and f"NST{nst} form1" in tag and tag.endswith(f"spread{spread}"), tag

    def launch(sel):
        for i in sel:
            if members[i][1] == "4a":
                outs[i].view.copy_(members[i][0].c0)
        _grouped([(members[i][0], members[i][1], outs[i], None) for i in sel], kn)
        res = []
        for i in sel:
            got, clean = outs[i].take()
            chk.true(f"{tag} member {i}", "wrote outside C's window", clean)
            res.append(got)
        return res
    together = launch(range(len(members)))
    for i, (o, epi) in enumerate(members):
        want = {"0": o.e["ref"].to(torch.bfloat16), "1": o.e["bias"].to(torch.bfloat16), "4": o.e["ref"].float(), "4a": o.e["acc"].float()}[epi]
        chk.bits(f"{tag} member {i} {o.m}x{o.n}x{o.k} epi{epi}", "against float64", together[i], want)
        if not (kn and epi == "1"):                # alone, a [K][N] weight takes no bias epilogue (gn_launch)
            chk.bits(f"{tag} member {i} {o.m}x{o.n}x{o.k} epi{epi}", "against its single launch", together[i], launch([i])[0])
        chk.true(f"{tag} member {i}", "an operand buffer changed", o.inputs_unchanged())
    torch.cuda.synchronize()
    print(f"\n[gemm_nt group {name}] {tag}, tile_end {tile_end}: {chk.n} checks, {len(chk.bad)} failed")
    chk.done()


def test_gemm_nt_grouped_refusals(gpu):
    """5 problems, epilogue 0 with a bias, epilogue 5 inside a group, and a bias epilogue on a lone [K][N] weight are refused."""
    from reformer_tts_amd import _lib
    o = _Ops(gpu, 128, 64, 64, 5, "int", t=64)
    c = _Win(gpu, 128, 64, torch.bfloat16, 72)
    delta = _Win(gpu, 2, 64, torch.float32)
    with pytest.raises(_lib.RttsError, match="1\\.\\.4 problems"):
        _grouped([(o, "0", c, None)] * 5, False)
    arr = (_lib.GemmNtProblem * 2)()
    for e in arr:
        _fill(e, o, False, "0", c)
        e.bias = o.bias.ptr
    for cnt in (1, 2):
        with pytest.raises(_lib.RttsError, match="takes no bias"):
            _lib.call("rtts_gemm_nt_grouped", arr, cnt, 0, _stream())
    with pytest.raises(_lib.RttsError, match="single-problem form"):
        _grouped([(o, "5", c, delta), (o, "0", c, None)], True)
    with pytest.raises(_lib.RttsError, match="epilogue 0, 3, 4 or 5"):
        _grouped([(o, "1", c, None)], True)
    torch.cuda.synchronize()
    assert bool((c.bits == c.pat).all()) and bool((delta.bits == delta.pat).all()), "a refused call wrote something"


# ------------------------------------------------------------------------------------------ normal inputs, one pass per tile
@pytest.mark.parametrize("name,m,n,nk", P.NORMAL, ids=[c[0] for c in P.NORMAL])
def test_gemm_nt_normal_inputs_elementwise_bound(gpu, name, m, n, nk):
    """N(0, 1) A, W scaled by K^-1/2, the path's deepest K: |got - ref| <= 2^-8 |ref| + 2^-16 scale elementwise for the bf16 epilogues
    (scale = |A| |W|^T, + |bias|, + |C0| where they enter), 2^-16 scale alone for the fp32 ones."""
    delta_t = 24 if "delta" in name else None
    k = 64 * nk
    o = _Ops(gpu, m, n, k, 4242 + nk, "normal", delta_t)
    e, sc = o.e, o.scale
    c16, c32 = _Win(gpu, m, n, torch.bfloat16, n + 8), _Win(gpu, m, n, torch.float32, n + 8)
    ratios = {}

    def score(key, got, ref, scale, bf16):
        ratios[key] = P.normal_ratio(got.double(), ref, scale, bf16)
    if delta_t is not None:
        delta = _Win(gpu, (m // delta_t) * (n // 64), delta_t, torch.float32)
        _grouped([(o, "5", c16, delta)], True)
        dout, clean = c16.take()
        score("kn 5 dout", dout, e["ref"], sc, True)
        dl, clean2 = delta.take()
        # delta is formed from the ROUNDED dout the kernel stored: against float64 on that dout, 64 fp32 products summed
        ops_out = o.out.view.double()
        want = (ops_out * dout.double()).view(m // delta_t, delta_t, n // 64, 64).sum(-1).permute(0, 2, 1).reshape(-1, delta_t)
        dscale = (ops_out.abs() * dout.double().abs()).view(m // delta_t, delta_t, n // 64, 64).sum(-1).permute(0, 2, 1).reshape(-1, delta_t)
        score("kn 5 delta", dl, want, dscale, False)
        assert clean and clean2
    else:
        for key, kn, epi, ref, scale in (("nt 0", False, "0", e["ref"], sc), ("nt 1", False, "1", e["bias"], sc + o.abs_bias),
                                         ("nt 2", False, "2", e["relu"], sc + o.abs_bias), ("kn 0", True, "0", e["ref"], sc),
                                         ("kn 3", True, "3", e["gated_table"], sc)):
            _single(o, kn, epi, c16, gate=o.gate if epi == "3" else None)
            got, clean = c16.take()
            assert clean, key
            score(key, got, ref, scale, True)
        for key, kn, epi, ref, scale in (("nt 4b", False, "4b", e["bias"], sc + o.abs_bias), ("kn 4", True, "4", e["ref"], sc)):
            _single(o, kn, epi, c32)
            got, clean = c32.take()
            assert clean, key
            score(key, got, ref, scale, False)
        c32.view.copy_(o.c0)
        _grouped([(o, "4a", c32, None)], False)
        got, clean = c32.take()
        assert clean
        score("nt 4a", got, e["ref"] + o.c0.double(), sc + o.abs_c0, False)
    torch.cuda.synchronize()
    worst = max(ratios, key=ratios.get)
    print(f"\n[gemm_nt normal {name} {m}x{n}x{k}] worst |err| / bound {ratios[worst]:.3f} ({worst}); " + ", ".join(f"{a} {b:.3f}" for a, b in ratios.items()))
    assert o.inputs_unchanged()
    assert ratios[worst] <= 1.0, ratios
