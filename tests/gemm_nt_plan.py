"""The host dispatcher of csrc/gemm_nt.hip restated in plain Python, the case list of tests/test_gemm_nt_exact_hip.py and the data
recipes both it and tests/test_gemm_nt_plan_cpu.py use.  No GPU and no library is needed to import or call anything here.

What is restated, with the lines of csrc/gemm_nt.hip it follows:
  gn_nst(bm, bn)            693-695   ring depth: as many 64-deep K stages of both operands as 160 KB of LDS hold, at most 4
  gn_store_mode(c, ldc)     730-734   16-byte (write-through) stores need a 16-byte aligned C and ldc % 8 == 0, else 8-byte stores
  gn_launch2                746-763   192 x 128: >= 512 tiles -> 2-deep ring (not for the fp32 / delta epilogues)
  gn_launch                 765-785   which epilogues each layout takes
  gn_launch_group           789-802   groups: 192 x 128 with more than 256 tiles -> 2-deep ring (`two`)
  gn_pick(M, N)             809-824   the tile of a single problem
  rtts_gemm_nt_partial_rows 826-829,  rtts_gemm_nt_gate_words 973-977
  rtts_gemm_nt_grouped      913-920   the tile of epilogue 5;  933-959 the tile of a group, its tile_end and `spread`
OUT OF SCOPE: the convolution forms (conv_cpt > 0: launch form 3, gn_conv_form) and epilogue 7; tests/test_conv_taps_hip.py owns
them.  Everything here is a plain GEMM: conv_cpt == 0.

A path tag reads  "<BM>x<BN><WM,WN> NST<n> form<0|1> <NT|KN> epi<e> st<s>[ spread<0|1>]":
  form   0 one problem, 1 grouped (one tile per workgroup in both)
  epi    0 plain, 1 bias, 2 bias + ReLU, 2w the same writing gate words, 3 ReLU gate from the activation, 3w from the words,
         4 fp32, 4b fp32 + bias, 4a fp32 accumulated into C, 5 input gradient + delta, 6 a group's run-time choice of 0 / 1 / 4
  st     the store form of a bf16 output (0 8-byte, 1 16-byte, 2 16-byte write-through), "f" for an fp32 output; a group lists
         its members' forms
If the dispatcher changes, tests/test_gemm_nt_plan_cpu.py fails instead of a path going untested."""

# ------------------------------------------------------------------------------------------ the dispatcher, restated
CAND = [(256, 256, 4), (192, 128, 4), (256, 128, 4), (96, 64, 2), (128, 64, 2)]          # BM, BN, WM (gn_cand); WN = 2
GN_MAX_GROUP = 4


def gn_pick(m, n):
    """Index into CAND of the tile a single (M, N) problem takes, or -1 (gn_pick, 809-824)."""
    best = -1
    for i in range(len(CAND)):
        bm, bn, _ = CAND[i]
        if m % bm or n % bn:
            continue
        wgs = (m // bm) * (n // bn)
        if i == 0 and wgs % 256 != 0:
            continue
        if best < 0:
            best = i
        if wgs >= 192:
            return i
    for i in (4, 3):
        if m % CAND[i][0] == 0 and n % CAND[i][1] == 0:
            return i
    return best


def gn_nst(bm, bn):
    lds = 160 * 1024
    return 4 if 4 * (bm + bn) * 128 <= lds else (3 if 3 * (bm + bn) * 128 <= lds else 2)


def partial_rows(m, n):
    i = gn_pick(m, n)
    return -1 if i < 0 else (m // CAND[i][0]) * CAND[i][2]


def gate_words(m, n):
    i = gn_pick(m, n)
    if i <= 0:
        return 0
    bm, bn, wm = CAND[i]
    return (m // bm) * (n // bn) * 64 * wm * 2


def gn_store_mode(c_addr, ldc, forced=-1):
    """``forced``: what rtts_debug_set_gemm_mode(10 + s) left (-1 = the library's pick, write-through)."""
    want = forced if forced >= 0 else 2
    return want if (c_addr & 15) == 0 and ldc % 8 == 0 else 0


def _st(epi, c_addr, ldc, forced):
    return "f" if str(epi).startswith("4") else str(gn_store_mode(c_addr, ldc, forced))


def _tag(bm, bn, wm, wn, nst, form, kn, epi, st, spread=None):
    t = f"{bm}x{bn}<{wm},{wn}> NST{nst} form{form} {'KN' if kn else 'NT'} epi{epi} st{st}"
    return t if spread is None else f"{t} spread{spread}"


# what gn_launch takes per layout.  Epilogue 3 on an [N][K] weight is legal there but nothing calls it (C = (A W^T) * gate is no layer
# of the model) and it is not listed; 4a and 5 come through rtts_gemm_nt_grouped with n = 1 only, where a [K][N] weight takes no 1
NT_EPIS = ("0", "1", "2", "2w", "4", "4b", "4a")
KN_EPIS = ("0", "3", "3w", "4", "4b", "4a", "5")


def nt_plan(m, n, k, kn=False, epi="0", c_addr=0, ldc=None, forced_store=-1):
    """The path of ONE plain problem through rtts_gemm_nt / rtts_gemm_nt_gated / rtts_gemm_nt_grouped(n = 1).  ``epi`` as in the
    module docstring; ``c_addr``, ``ldc`` where C lies.  -> path tag."""
    epi = str(epi)
    assert k > 0 and k % 64 == 0 and epi in (KN_EPIS if kn else NT_EPIS), (k, kn, epi)
    ldc = n if ldc is None else ldc
    if epi == "5":                                                       # 913-920
        assert kn
        if m % 192 == 0 and n % 128 == 0 and (m // 192) * (n // 128) >= 192:
            bm, bn, wm, wn = 192, 128, 4, 2
        elif m % 128 == 0 and n % 64 == 0:
            bm, bn, wm, wn = 128, 64, 4, 1
        elif m % 192 == 0 and n % 128 == 0:
            bm, bn, wm, wn = 192, 128, 4, 2
        else:
            raise ValueError(f"epilogue 5 does not tile {m} x {n}")
    else:
        i = gn_pick(m, n)
        if i < 0:
            raise ValueError(f"no tile for {m} x {n}")
        if epi in ("2w", "3w") and i == 0:
            raise ValueError("256 x 256 has no gate words")
        (bm, bn, wm), wn = CAND[i], 2
    nst = gn_nst(bm, bn)
    if (bm, bn) == (192, 128) and epi[0] not in "45" and (m // bm) * (n // bn) >= 512:      # 756-761
        nst = 2
    return _tag(bm, bn, wm, wn, nst, 0, kn, epi, _st(epi, c_addr, ldc, forced_store))


def group_plan(problems, kn=False, forced_store=-1):
    """rtts_gemm_nt_grouped with n > 1.  ``problems``: (M, N, K, epi, c_addr, ldc) each -> (path tag, tile_end).  933-959, 789-802."""
    assert 2 <= len(problems) <= GN_MAX_GROUP

    def tiles_by(bm, bn):
        t = 0
        for m, n, *_ in problems:
            if m % bm or n % bn:
                return -1
            t += (m // bm) * (n // bn)
        return t
    bm, bn, total = 192, 128, tiles_by(192, 128)
    if total < 192:
        t96, t128 = tiles_by(96, 64), tiles_by(128, 64)
        if t96 > 0:
            bm, bn, total = 96, 64, t96
        elif t128 > 0:
            bm, bn, total = 128, 64, t128
    if total <= 0:
        raise ValueError("the problems share no tile shape")
    counts = [(m // bm) * (n // bn) for m, n, *_ in problems]
    spread = int(all(t % 8 == 0 for t in counts))
    tile_end = [sum(counts[:i + 1]) for i in range(len(counts))]
    nst = 2 if bm == 192 and total > 256 else gn_nst(bm, bn)
    wm = 4 if bm == 192 else 2
    st = ",".join(_st(e, c, ld, forced_store) for _, _, _, e, c, ld in problems)
    return _tag(bm, bn, wm, 2, nst, 1, kn, "6", st, spread), tile_end


# ------------------------------------------------------------------------------------------ the reachable paths
def reachable_plain_tags():
    """Every path tag a plain single problem can take, enumerated from the STRUCTURE of the dispatcher (which tile has which
    ring depths, launch forms, epilogues and store forms), not from the case list:
      * 192 x 128 runs its deep ring below 512 tiles and the 2-deep ring from 512 tiles on (bf16 epilogues only); every other
        tile has one ring depth; a single problem is form 0;
      * 256 x 256 has no gate words; epilogue 5 runs on 192 x 128 <4,2> and on 128 x 64 as <4,1>, deep ring;
      * a bf16 output is stored in form 2 (aligned) or 0 (not), and in form 1 on request."""
    tags = set()
    for i, (bm, bn, wm) in enumerate(CAND):
        rings = [gn_nst(bm, bn)]
        for kn, epis in ((False, NT_EPIS), (True, KN_EPIS)):
            for epi in epis:
                if epi == "5" or (i == 0 and epi.endswith("w")):
                    continue
                r = list(rings)
                if (bm, bn) == (192, 128) and epi[0] != "4":
                    r.append(2)
                for nst in r:
                    for st in (("f",) if epi[0] == "4" else ("0", "1", "2")):
                        tags.add(_tag(bm, bn, wm, 2, nst, 0, kn, epi, st))
    for bm, bn, wm, wn in ((192, 128, 4, 2), (128, 64, 4, 1)):
        for st in ("0", "1", "2"):
            tags.add(_tag(bm, bn, wm, wn, 4, 0, True, "5", st))
    return tags


# ------------------------------------------------------------------------------------------ the GPU case list
def _nks(nst):
    return sorted({1, nst - 1, nst, nst + 1, 2 * nst + 1})


# name (goes into the test id) -> what the case runs.  ``shapes``: (M, N) each; ``nks``: K = 64 nk; ``delta``: the T of an
# epilogue-5 run per shape (None: the shape runs the plain epilogues).  "192x128_persistent" keeps the name it had when it also ran
# the persistent launch forms: 1024 tiles (four per CU) on the 2-deep ring, at K of 4, 5 and 9 stages
CASES = {
    "256x256_nst2": dict(shapes=[(8192, 2048)], nks=_nks(2), tile=(256, 256), nst=2),
    "192x128_nst4": dict(shapes=[(3072, 1536)], nks=_nks(4), tile=(192, 128), nst=4),
    "192x128_nst2": dict(shapes=[(6144, 2048)], nks=_nks(2), tile=(192, 128), nst=2),
    "192x128_persistent": dict(shapes=[(6144, 4096)], nks=[4, 5, 9], tile=(192, 128), nst=2),
    "256x128_nst3": dict(shapes=[(4096, 1536)], nks=_nks(3), tile=(256, 128), nst=3),
    "96x64_nst4": dict(shapes=[(96, 64), (192, 128), (288, 64), (1536, 768)], nks=_nks(4), tile=(96, 64), nst=4),
    "128x64_nst4": dict(shapes=[(128, 64), (384, 256), (2048, 768)], nks=_nks(4), tile=(128, 64), nst=4),
    "delta_128x64_w41": dict(shapes=[(512, 128), (384, 256)], delta=[256, 24], nks=_nks(4), tile=(128, 64), nst=4),
    "delta_192x128": dict(shapes=[(3072, 1536), (192, 128), (192, 128), (576, 256)], delta=[256, 24, 192, 64], nks=_nks(4),
                          tile=(192, 128), nst=4),
}
CASE_IDS = [f"{name}-nk{nk}" for name, c in CASES.items() for nk in c["nks"]]
CASE_PARAMS = [(name, nk) for name, c in CASES.items() for nk in c["nks"]]

# the three placements of C (offset of the window into its 16-byte aligned buffer in BYTES, extra leading-dimension elements) and
# the store form each must take, then the two forced forms on the aligned placement: (name, byte offset, ldc - N, debug mode)
PLACEMENTS = [("aligned", 0, 8, 9), ("plus8bytes", 8, 8, 9), ("ldc_mod8_is4", 0, 4, 9), ("forced1", 0, 8, 11), ("forced2", 0, 8, 12)]
EXPECTED_STORE = {"aligned": "2", "plus8bytes": "0", "ldc_mod8_is4": "0", "forced1": "1", "forced2": "2"}
SINGLE_NT = ("0", "1", "2", "2w", "4", "4b")                 # through rtts_gemm_nt / rtts_gemm_nt_gated
SINGLE_KN = ("0", "3", "3w", "4", "4b")
GROUPED_N1_NT = ("0", "1", "4", "4a")                        # through rtts_gemm_nt_grouped, n = 1
GROUPED_N1_KN = ("0", "4", "4a")                             # (+ 5 in the delta cases)


def case_tags(name, nk):
    """Every path tag the GPU test of (name, nk) runs (the same calls, in the same placements, as _run_plain / _run_delta there)."""
    c, k, tags = CASES[name], 64 * nk, set()
    for idx, (m, n) in enumerate(c["shapes"]):
        for pl, off, pad, dbg in PLACEMENTS:
            forced = dbg - 10 if dbg >= 10 else -1
            if "delta" in c:
                tags.add(nt_plan(m, n, k, True, "5", off, n + pad, forced))
                continue
            words = gate_words(m, n) > 0
            for kn, epis in ((False, SINGLE_NT + GROUPED_N1_NT), (True, SINGLE_KN + GROUPED_N1_KN)):
                for epi in epis:
                    if epi.endswith("w") and not words:
                        continue
                    if epi[0] == "4" and off:
                        continue                     # an fp32 C is 16-byte aligned by contract
                    tags.add(nt_plan(m, n, k, kn, epi, off, n + pad, forced))
    return tags


def all_case_tags():
    out = {}
    for name, nk in CASE_PARAMS:
        for t in case_tags(name, nk):
            out.setdefault(t, []).append(f"{name}-nk{nk}")
    return out


# groups: name -> members (M, N, K, epi); run in both layouts.  Tile counts in the comments are by the group's tile.
GROUPS = {
    "192x128_two_nst4_spread": [(1536, 1536, 256, "0"), (1536, 1536, 320, "1")],                               # 96 + 96 = 192
    "192x128_three_nst2_spread": [(1536, 1536, 64, "0"), (1536, 1536, 128, "1"), (1536, 1536, 192, "4")],      # 288
    "192x128_four_nst2_nospread": [(1536, 1536, 64, "0"), (1536, 1536, 128, "1"), (1536, 1536, 192, "4"), (960, 384, 320, "0")],  # 303
    "192x128_three_nst4_nospread": [(1536, 1536, 192, "0"), (1536, 1536, 320, "1"), (960, 384, 576, "4")],     # 207
    "96x64_spread": [(768, 64, 192, "0"), (384, 256, 256, "1"), (96, 512, 320, "4")],                          # 8, 16, 8
    "96x64_nospread": [(288, 64, 64, "1"), (192, 192, 256, "0"), (96, 64, 576, "4")],                          # 3, 6, 1
    "128x64_spread": [(512, 128, 192, "1"), (256, 256, 64, "0"), (1024, 64, 320, "4")],                        # 8, 8, 8
    "128x64_nospread": [(128, 64, 320, "0"), (640, 192, 256, "4"), (256, 128, 192, "1")],                      # 1, 15, 4
    "four_mixed_k_and_epilogues": [(288, 128, 64, "0"), (192, 64, 192, "1"), (96, 192, 320, "4"), (384, 128, 576, "4a")],
}
GROUP_EXPECT = {        # name -> (tile, NST, spread): what the issue asks each group to reach
    "192x128_two_nst4_spread": ("192x128", 4, 1), "192x128_three_nst2_spread": ("192x128", 2, 1),
    "192x128_four_nst2_nospread": ("192x128", 2, 0), "192x128_three_nst4_nospread": ("192x128", 4, 0),
    "96x64_spread": ("96x64", 4, 1), "96x64_nospread": ("96x64", 4, 0), "128x64_spread": ("128x64", 4, 1),
    "128x64_nospread": ("128x64", 4, 0), "four_mixed_k_and_epilogues": ("96x64", 4, 0),
}

# one normal-input pass per tile: (name, M, N, nk = the path's largest, kn layout run too, T of a delta run or None)
NORMAL = [("256x256", 8192, 2048, 5), ("192x128_nst4", 3072, 1536, 9), ("192x128_nst2", 6144, 2048, 5), ("256x128", 4096, 1536, 7),
          ("96x64", 1536, 768, 9), ("128x64", 2048, 768, 9), ("128x64_w41_delta", 384, 256, 9)]


# ------------------------------------------------------------------------------------------ exactness conditions
A_MAX, BIAS_MAX, OUT_MAX = 4, 64, 4


def exactness(k, tile):
    """The conditions under which fp32 holds every partial sum exactly, whatever the order (all operands are integers):
      product    |sum_k a w| + |bias or C0| <= 16 K + 64 < 2^24;
      colsum     a partial row is the fp32 sum of the gated product over ONE wave's BM / WM rows: (BM / WM) 16 K < 2^24 (the
                 test adds the partial rows in float64; M 16 K < 2^24 -- what one fp32 sum over all M rows would need -- holds
                 for none of the large shapes and is not needed: no kernel here forms that sum);
      delta      64 columns of |out| <= 4 times |bf16(dout)| <= 16 K (1 + 2^-8): 64 * 4 * 16 K (1 + 2^-8) < 2^24.
    -> dict of the three left-hand sides."""
    wm = next(w for bm, bn, w in CAND if (bm, bn) == tuple(tile))
    return dict(product=A_MAX * A_MAX * k + BIAS_MAX, colsum=(tile[0] // wm) * A_MAX * A_MAX * k,
                delta=64 * OUT_MAX * A_MAX * A_MAX * k * (1 + 2.0 ** -8))


# ------------------------------------------------------------------------------------------ data recipes (torch; any device)
GATE_TABLE_BITS = [0xC000, 0x8000, 0x0000, 0x0001, 0x3F80, 0x4040]     # bf16: -2, -0.0, +0.0, the smallest subnormal, 1, 3
GATE_TABLE_OPEN = [False, False, False, True, True, True]               # is the value > 0


def int_operands(m, n, k, seed, device):
    """The exact recipe: A (M, K), W (N, K) integers in [-4, 4]; bias (N,), C0 (M, N) integers in [-64, 64]; out (M, N) integers in
    [-4, 4]; gate index (M, N) into GATE_TABLE_*.  All float64 but the index."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g, device=device).double()
    return dict(a=ri(-4, 4, m, k), w=ri(-4, 4, n, k), bias=ri(-64, 64, n), c0=ri(-64, 64, m, n), out=ri(-4, 4, m, n),
                gate_idx=torch.randint(0, 6, (m, n), generator=g, device=device))


def normal_operands(m, n, k, seed, device):
    """The normal recipe: A ~ N(0, 1), W ~ N(0, 1) / sqrt(K), both rounded to bf16 (returned as float64); bias, C0 ~ N(0, 1) fp32."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    a = torch.randn(m, k, generator=g, device=device).bfloat16().double()
    w = (torch.randn(n, k, generator=g, device=device) / k ** 0.5).bfloat16().double()
    return dict(a=a, w=w, bias=torch.randn(n, generator=g, device=device).double(), c0=torch.randn(m, n, generator=g, device=device).double(),
                out=torch.randn(m, n, generator=g, device=device).bfloat16().double(),
                gate_idx=torch.randint(0, 6, (m, n), generator=g, device=device))


def gate_open(gate_idx):
    import torch
    return torch.tensor(GATE_TABLE_OPEN, device=gate_idx.device)[gate_idx]


def expectations(ops, t=None):
    """float64 expectations of every epilogue on one set of operands: product, + bias, relu(+ bias), gated by the table gate,
    gated by h = bf16(relu(+ bias)) > 0, column sums of both gated products, + C0; with ``t``: delta (B * H, T) of epilogue 5 on
    dout = bf16(product)."""
    import torch
    ref = ops["a"] @ ops["w"].t()
    e = dict(ref=ref, bias=ref + ops["bias"], relu=torch.relu(ref + ops["bias"]), acc=ref + ops["c0"], acc_bias=ref + ops["bias"] + ops["c0"])
    e["h_open"] = e["relu"].to(torch.bfloat16) != 0
    # (a closed gate stores +0.0 whatever the sign of the product: select, do not multiply -- -3 * 0 is -0.0)
    zero = torch.zeros_like(ref)
    e["gated_table"] = torch.where(gate_open(ops["gate_idx"]), ref, zero)
    e["gated_h"] = torch.where(e["h_open"], ref, zero)
    e["colsum_table"], e["colsum_h"] = e["gated_table"].sum(0), e["gated_h"].sum(0)
    if t is not None:
        m, n = ref.shape
        dout = ref.to(torch.bfloat16).double()
        e["delta"] = (ops["out"] * dout).view(m // t, t, n // 64, 64).sum(-1).permute(0, 2, 1).reshape(-1, t)
    return e


NORMAL_BF16_TERM, NORMAL_F32_TERM = 2.0 ** -8, 2.0 ** -16


def normal_ratio(got, ref, scale, bf16):
    """max over elements of |got - ref| / (2^-8 |ref| + 2^-16 scale) (bf16 output: half an ulp of the result + the margin over
    fp32 summation noise tests/test_gemm_tn_hip.py uses: ~2^-24 of ``scale`` = |A| |W|^T (+ |bias| ...) per addition, a few hundred
    additions at most, against one k column's share of it, ~1 / K >= 2^-10) or / (2^-16 scale) (fp32 output).  <= 1 passes."""
    bound = NORMAL_F32_TERM * scale
    if bf16:
        bound = bound + NORMAL_BF16_TERM * ref.abs()
    return ((got - ref).abs() / bound).max().item()


# ------------------------------------------------------------------------------------------ the gate words' lane -> element map
def decode_gate_words(words, m, n):
    """(M, N) bool from the words epilogue 2 writes, by the map documented at kBitsFit (csrc/gemm_nt.hip:505-510, 481, 126): word
    (tile_m * (N / BN) + tile_n) * 64 WM WN + tid, tid = 64 (wm * WN + wn) + 16 g + r; bit (i * TN + j) * 4 + e <=> row
    tile_m BM + wm (BM / WM) + 16 i + r, column tile_n BN + wn (BN / WN) + 16 j + 4 g + e.  -> (mask, are all bits
    from 4 TM TN upwards clear)."""
    import torch
    bm, bn, wm = CAND[gn_pick(m, n)]
    wn = 2
    tm, tn = bm // wm // 16, bn // wn // 16
    w = words.view(m // bm, n // bn, wm, wn, 4, 16)                       # tile_m, tile_n, wm, wn, g, r
    sh = torch.arange(tm * tn * 4, device=words.device).view(tm, tn, 4)     # i, j, e
    bits = ((w[..., None, None, None] >> sh) & 1).bool()                    # tile_m, tile_n, wm, wn, g, r, i, j, e
    mask = bits.permute(0, 2, 6, 5, 1, 3, 7, 4, 8).reshape(m, n)            # tile_m, wm, i, r | tile_n, wn, j, g, e
    nbits = tm * tn * 4
    high_clear = True if nbits == 64 else bool(((words >> nbits) == 0).all())
    return mask, high_clear
