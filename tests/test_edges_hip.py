"""The BatchNorm, positional-encoding, relu-dropout and layout kernels of csrc/edges.hip through the C ABI (``_lib.call``) against the
float64 references of tests/edges_ref.py (themselves checked on the CPU by tests/test_edges_ref_cpu.py).

Conventions of every test here: halo rows, lead-in and tail of every INPUT halo array hold NaN (a kernel that reads one fails
loudly), every OUTPUT is prefilled with 7.0 and must come back zero outside its valid rows; dropout masks are rebuilt on the host
from oracle.synth.drop_hash, never recovered from a kernel's output.

Bounds (u = 2^-24, r = |mean| / std of a channel in float64):
  mean        2^-18 * mean|y|                       add chains of at most 64 float32 additions
  rstd        16 u (1 + r^2) relative               var = q/M - mu^2 from raw single-pass sums: the two terms carry a few roundings
                                                    at magnitude mean^2 + var, the difference amplifies them by 1 + r^2, the inverse
                                                    square root halves them ("BatchNorm variance")
  running     the two bounds above carried through  0.9 old + 0.1 new  (+ 4 u of the formula's own roundings); a relative error e of
              rstd is an absolute error 2 e (var + eps) of var
  z           2^-8 |z64| + 2e-6                     bf16 half-ulp + the fast tanh.  bf16 keeps 8 significant bits: rounding to nearest
                                                    is off by up to 2^-8 of the value (1 + 2^-8 lies exactly between 1 and 1 + 2^-7),
                                                    so 2^-9 cannot be met by ANY bf16 output; measured worst 1.99 * 2^-9 on every shape
  dy          2^-8 |dy64| + 2e-5 max|dy64| + 8 u (the three terms of dy), see _dy_tol
  dgamma/beta 2^-18 * sum|terms|  (+ u |result|: the one addition into the non-zero starting value)
  pe_add      4 u (|y| + |alpha table| / (1-p));   pe_dalpha 2^-18 * sum|dy table keep|;   relu_drop 2^-9 |ref|;   layouts bit-exact
ReLU: elements with |pre64| < 1e-5 (1 + |beta|), where float32 may flip the gate, are left out; they must be < 0.1 % of a case.

Measured on an MI355X, worst |kernel - float64| / bound over the whole file (must be <= 1):
    rstd 0.33 (0.30 from host-made partial rows, 0.23 through the convolution's epilogue)   mean 0.07   running mean 0.29  var 0.35
    z 0.996 and dy 0.98 (bf16 rounding to nearest: the bound is tight by construction)      dgamma 0.21   dbeta 0.11
    pe_add 0.63   pe_dalpha 0.013   relu_drop and the layout kernels exact; the whole file runs in about 6 s."""
import numpy as np
import pytest
import torch

import edges_ref as R

pytestmark = pytest.mark.gpu

U = R.U24
LEAD, TAIL = 8, 11            # lead-in and tail rows of the halo outputs under test
PBLOCKS = 256                 # ED_PBLOCKS of csrc/edges.hip: partial rows of the column sums


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__
    __graft_entry__.build()
    return torch.device("cuda:0")


def _call(name, *args):
    from reformer_tts_amd import _lib
    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _f64(t):
    return t.detach().float().cpu().double().numpy()


# ------------------------------------------------------------------ halo layout helpers (host side)
def _valid_rows(b, l, halo, lead=0):
    """indices of the B*L data rows of a halo array whose halo row 0 is row `lead`."""
    return (lead + np.arange(b)[:, None] * (l + 2 * halo) + halo + np.arange(l)[None, :]).reshape(-1)


def _to_halo(x, b, l, halo, junk, lead=0, tail=0):
    """x (B*L, C) -> (lead + B*(L+2*halo) + tail, C) of the same dtype, `junk` everywhere but the data rows."""
    out = torch.full((lead + b * (l + 2 * halo) + tail, x.shape[1]), junk, dtype=x.dtype)
    out[torch.from_numpy(_valid_rows(b, l, halo, lead))] = x
    return out


def _split_halo(xh, b, l, halo, lead=0):
    """device halo array -> (data rows (B*L, C), the other rows), both on the CPU."""
    xh = xh.cpu()
    sel = torch.zeros(xh.shape[0], dtype=torch.bool)
    sel[torch.from_numpy(_valid_rows(b, l, halo, lead))] = True
    return xh[sel], xh[~sel]


def _ws(gpu, c):
    return torch.full(((2 * PBLOCKS + 2) * c + 1,), float("nan"), device=gpu)


# ================================================================== A. statistics
STAT_GEOS = [(1, 2, 0, 4), (3, 5, 2, 8), (2, 131, 2, 64), (3, 200, 2, 320), (2, 700, 2, 64), (2, 64, 0, 512)]
R_GRID = [0, 1, 8, 32, 128]
_ys = {}


def _stat_input(b, l, c, r):
    """y (B*L, C) float32 = sign_c r s_c + s_c randn, s_c log-uniform in [0.1, 10]; shared by the tests of one (geometry, r)."""
    key = (b, l, c, r)
    if key not in _ys:
        gen = torch.Generator().manual_seed(1000 * r + b * l + c)
        s = 10.0 ** (torch.rand(c, generator=gen) * 2.0 - 1.0)
        sign = torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0)
        _ys[key] = (sign * r * s + s * torch.randn(b * l, c, generator=gen)).float()
    return _ys[key]


class _Stats:
    """float64 statistics of y (M, C) float32 and the bounds that go with them."""

    def __init__(self, y):
        y64 = y.double().numpy()
        self.m = y64.shape[0]
        self.mean, self.var, self.rstd = R.bn_stats(y64)
        self.r = np.abs(self.mean) * self.rstd
        self.mean_tol = 2.0 ** -18 * np.abs(y64).mean(0)
        self.rstd_tol = 16 * U * (1 + self.r ** 2)

    def check(self, mean, rstd, what):
        """-> (worst mean error / bound, worst rstd relative error, worst rstd error / bound)."""
        em = np.abs(_f64(mean) - self.mean)
        er = np.abs(_f64(rstd) / self.rstd - 1)
        i, k = int((em / np.maximum(self.mean_tol, 1e-300)).argmax()), int((er / self.rstd_tol).argmax())
        assert (em <= self.mean_tol).all(), (what, "mean", i, em[i], self.mean_tol[i])
        assert (er <= self.rstd_tol).all(), (what, "rstd", k, er[k], self.rstd_tol[k], self.r[k])
        return float((em / np.maximum(self.mean_tol, 1e-300)).max()), float(er.max()), float((er / self.rstd_tol).max())

    def check_running(self, rm, rv, rm0, rv0, shift, what):
        want_m, want_v = R.bn_running(rm0, rv0, self.mean, self.var, self.m, shift)
        sh = 0.0 if shift is None else np.abs(shift)
        tol_m = 0.1 * self.mean_tol + 4 * U * (0.9 * np.abs(rm0) + 0.1 * (np.abs(self.mean) + sh))
        unb = self.m / max(self.m - 1, 1)
        tol_v = 0.1 * unb * 2 * self.rstd_tol * (self.var + R.EPS) + 4 * U * (0.9 * np.abs(rv0) + 0.1 * unb * self.var)
        em, ev = np.abs(_f64(rm) - want_m), np.abs(_f64(rv) - want_v)
        assert (em <= tol_m).all(), (what, "running_mean", float((em / tol_m).max()))
        assert (ev <= tol_v).all(), (what, "running_var", float((ev / tol_v).max()))
        return float((em / tol_m).max()), float((ev / tol_v).max())


def _run_stats(gpu, path, yh, b, l, halo, c, rm0, rv0, shift, with_count, count=None):
    """One statistics launch by `path` ('stats' | 'moments') -> mean, rstd, running mean, running var, num_batches (device)."""
    mean, rstd = torch.full((c,), 7.0, device=gpu), torch.full((c,), 7.0, device=gpu)
    rm, rv = torch.from_numpy(rm0).float().to(gpu), torch.from_numpy(rv0).float().to(gpu)
    sh = None if shift is None else torch.from_numpy(shift).float().to(gpu)
    nbt = torch.tensor([4], dtype=torch.int64, device=gpu) if with_count else None
    ws = _ws(gpu, c)
    if path == "stats":
        _call("rtts_bn_stats", yh.data_ptr(), b, l, halo, c, mean.data_ptr(), rstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), _ptr(sh), _ptr(nbt),
              ws.data_ptr())
    else:
        mom = torch.full((2 * c + 1,), 7.0, device=gpu)
        _call("rtts_bn_moments", yh.data_ptr(), b, l, halo, c, mom.data_ptr(), ws.data_ptr())
        assert float(mom[2 * c]) == 7.0                       # the count slot belongs to the caller
        _call("rtts_bn_from_moments", mom.data_ptr(), b * l if count is None else count, c, mean.data_ptr(), rstd.data_ptr(), rm.data_ptr(),
              rv.data_ptr(), _ptr(sh), _ptr(nbt))
    torch.cuda.synchronize()
    if with_count:
        assert int(nbt) == 5
    return mean, rstd, rm, rv


def _running_start(c, seed):
    rs = np.random.RandomState(seed)
    f = np.float32
    return (rs.standard_normal(c).astype(f).astype(np.float64), (0.5 + rs.rand(c)).astype(f).astype(np.float64),
            rs.standard_normal(c).astype(f).astype(np.float64))


@pytest.mark.parametrize("r", R_GRID)
@pytest.mark.parametrize("b,l,halo,c", STAT_GEOS)
def test_bn_statistics_vs_float64(gpu, b, l, halo, c, r):
    """rtts_bn_stats and rtts_bn_moments + rtts_bn_from_moments(count = B*L): mean, rstd and running statistics (mean_shift and
    num_batches given and absent) against float64; the two paths bit for bit equal (same sums, same formula)."""
    y = _stat_input(b, l, c, r)
    st = _Stats(y)
    yh = _to_halo(y, b, l, halo, float("nan")).to(gpu)
    rm0, rv0, shift = _running_start(c, c + r)
    out = {}
    for path in ("stats", "moments"):
        for sh, cnt in ((shift, True), (None, False)):
            mean, rstd, rm, rv = _run_stats(gpu, path, yh, b, l, halo, c, rm0, rv0, sh, cnt)
            em, er, ratio = st.check(mean, rstd, path)
            erm, erv = st.check_running(rm, rv, rm0, rv0, sh, path)
            out[path, cnt] = (mean, rstd, rm, rv)
        print(f"\n[bn statistics] path={path} {b}x{l}x{c} halo {halo} r={r}: rstd rel err {er:.2e} = {ratio:.3f} of its bound, mean {em:.3f}, "
              f"running mean {erm:.3f} var {erv:.3f} of theirs (tol 1)")
    for cnt in (True, False):
        for a, bb, name in zip(out["stats", cnt], out["moments", cnt], ("mean", "rstd", "running_mean", "running_var")):
            assert torch.equal(a, bb), f"rtts_bn_from_moments differs from rtts_bn_stats in {name}"


@pytest.mark.parametrize("b,l,halo,c", STAT_GEOS)
def test_bn_statistics_constant_channel(gpu, b, l, halo, c):
    """A channel that is constant (1000.25: its square and every partial sum of it are exact in float32 below 4193 rows): the
    raw-moment variance cancels to rounding noise, which must not turn into a NaN or a huge rstd; the mean is exact."""
    y = _stat_input(b, l, c, 1).clone()
    y[:, 1] = 1000.25
    yh = _to_halo(y, b, l, halo, float("nan")).to(gpu)
    rm0, rv0, _ = _running_start(c, 3)
    top = (1.0 / np.sqrt(np.float64(np.float32(1e-5)))) * (1 + 1e-6)
    for path in ("stats", "moments"):
        mean, rstd, rm, rv = _run_stats(gpu, path, yh, b, l, halo, c, rm0, rv0, None, False)
        assert float(mean[1]) == 1000.25
        assert np.isfinite(_f64(rstd)).all() and 0 < float(rstd[1]) <= top, float(rstd[1])
        assert np.isfinite(_f64(rv)).all() and np.isfinite(_f64(rm)).all()
    print(f"\n[bn statistics] constant channel {b}x{l}x{c}: rstd {float(rstd[1]):.4f} (tol <= {top:.4f})")


@pytest.mark.parametrize("r", R_GRID)
@pytest.mark.parametrize("b,l,halo,c", [g for g in STAT_GEOS if g[0] == 3])
def test_bn_statistics_two_simulated_ranks(gpu, b, l, halo, c, r):
    """Data-parallel BatchNorm without the second process: one moments vector per part of the batch (2 + 1 samples) with its row count
    in slot 2C, the two added as an all-reduce would, rtts_bn_from_moments(count = 0) -> the statistics of the whole batch."""
    y = _stat_input(b, l, c, r)
    st = _Stats(y)
    total = torch.zeros(2 * c + 1, device=gpu)
    for lo, hi in ((0, 2), (2, 3)):
        part = _to_halo(y[lo * l:hi * l], hi - lo, l, halo, float("nan")).to(gpu)
        mom = torch.full((2 * c + 1,), 7.0, device=gpu)
        _call("rtts_bn_moments", part.data_ptr(), hi - lo, l, halo, c, mom.data_ptr(), _ws(gpu, c).data_ptr())
        mom[2 * c] = float((hi - lo) * l)
        total += mom
    rm0, rv0, shift = _running_start(c, r)
    mean, rstd = torch.full((c,), 7.0, device=gpu), torch.full((c,), 7.0, device=gpu)
    rm, rv = torch.from_numpy(rm0).float().to(gpu), torch.from_numpy(rv0).float().to(gpu)
    sh = torch.from_numpy(shift).float().to(gpu)
    _call("rtts_bn_from_moments", total.data_ptr(), 0, c, mean.data_ptr(), rstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), sh.data_ptr(), None)
    torch.cuda.synchronize()
    em, er, ratio = st.check(mean, rstd, "two ranks")
    erm, erv = st.check_running(rm, rv, rm0, rv0, shift, "two ranks")
    print(f"\n[bn statistics] path=two-ranks {b}x{l}x{c} halo {halo} r={r}: rstd rel err {er:.2e} = {ratio:.3f} of its bound, mean {em:.3f}, "
          f"running mean {erm:.3f} var {erv:.3f} of theirs (tol 1)")


@pytest.mark.parametrize("c", [4, 64, 320])
@pytest.mark.parametrize("nrows", [1, 15, 16, 17, 255, 256, 257, 600])
def test_bn_stats_from_partials_vs_float64(gpu, nrows, c):
    """rtts_bn_stats_from_partials on partial rows made on the host (float64 sums of row groups, rounded to float32) at the boundaries
    of the 16-wave x 16-row pass of the finalize kernel; the reference is float64 on the same rounded partials."""
    m = 2 * nrows + 5
    gen = torch.Generator().manual_seed(nrows * 1000 + c)
    rr = torch.tensor(R_GRID, dtype=torch.float32)[torch.arange(c) % len(R_GRID)]
    s = 10.0 ** (torch.rand(c, generator=gen) * 2.0 - 1.0)
    sign = torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0)
    y = (sign * rr * s + s * torch.randn(m, c, generator=gen)).float().double().numpy()
    groups = np.array_split(np.arange(m), nrows)
    part = np.stack([np.concatenate([y[g].sum(0), (y[g] ** 2).sum(0)]) for g in groups]).astype(np.float32)
    # a row behind the last: a finalize that read one row too many would not get past it
    pd = torch.from_numpy(np.concatenate([part, np.full((1, 2 * c), np.nan, np.float32)])).to(gpu)
    p64 = part.astype(np.float64).sum(0)
    st = _Stats.__new__(_Stats)
    st.m = m
    st.mean = p64[:c] / m
    st.var = p64[c:] / m - st.mean ** 2
    st.rstd = 1.0 / np.sqrt(st.var + R.EPS)
    st.r = np.abs(st.mean) * st.rstd
    st.mean_tol = 2.0 ** -18 * np.abs(y).mean(0)
    st.rstd_tol = 16 * U * (1 + st.r ** 2)
    rm0, rv0, shift = _running_start(c, nrows)
    mean, rstd = torch.full((c,), 7.0, device=gpu), torch.full((c,), 7.0, device=gpu)
    rm, rv = torch.from_numpy(rm0).float().to(gpu), torch.from_numpy(rv0).float().to(gpu)
    sh, nbt = torch.from_numpy(shift).float().to(gpu), torch.tensor([4], dtype=torch.int64, device=gpu)
    _call("rtts_bn_stats_from_partials", pd.data_ptr(), nrows, 1, m, c, mean.data_ptr(), rstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), sh.data_ptr(),
          nbt.data_ptr())
    torch.cuda.synchronize()
    assert int(nbt) == 5
    em, er, ratio = st.check(mean, rstd, "from partials")
    erm, erv = st.check_running(rm, rv, rm0, rv0, shift, "from partials")
    print(f"\n[bn statistics] path=from-partials {nrows} rows x {c}: rstd rel err {er:.2e} = {ratio:.3f} of its bound, mean {em:.3f}, "
          f"running mean {erm:.3f} var {erv:.3f} of theirs (tol 1)")


@pytest.mark.parametrize("kind", ["randn", "ones", "ones-taps-full", "ones-taps-full-0.2"])
@pytest.mark.parametrize("b,l,ci,co", [(1, 64, 64, 64), (2, 131, 80, 512)])
def test_conv_epilogue_moments_vs_float64(gpu, b, l, ci, co, kind):
    """The convolution's own epilogue (rtts_conv1d_k5_moments through edges.ConvK5.forward_moments) + rtts_bn_stats_from_partials
    against float64 statistics of the y the kernel itself wrote.
      randn               plain input, r below 1
      ones                1 + 0.02 randn through all-positive weights.  The zero padding caps r: the two rows at either end of a
                          sequence see 3 and 4 of the 5 taps, their outputs sit at 0.6 and 0.8 of the mean, and that alone is a
                          std of mean * sqrt(0.4 / L): r = 12.7 at L = 64 and 18 at L = 131 whatever the noise (float64 convolution
                          on the CPU).  This is the largest r a zero-padded sequence of this length reaches; reported, not asserted.
      ones-taps-full      the same input ALSO in the two halo rows around every sequence (an implicit GEMM reads whatever the halo
                          rows hold), so every output row sees five taps: r about 800; asserted >= 30 on half the channels.
      ones-taps-full-0.2  noise 0.2 instead of 0.02: r about 77, where the bound is not yet vacuous."""
    from reformer_tts_amd import edges
    gen = torch.Generator().manual_seed(b * l + ci)
    conv = torch.nn.Conv1d(ci, co, 5, padding=2)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(co, ci, 5, generator=gen) / (5 * ci) ** 0.5)
        if kind != "randn":
            conv.weight.abs_()
    conv = conv.to(gpu)
    g = edges.Halo(b, l)
    sigma = 0.2 if kind.endswith("0.2") else 0.02
    x = torch.randn(b, g.p, ci, generator=gen) if kind == "randn" else 1 + sigma * torch.randn(b, g.p, ci, generator=gen)
    if "full" not in kind:
        x[:, :g.H] = 0
        x[:, g.H + l:] = 0
    ex = edges.ConvK5(conv)
    xh = torch.zeros(g.alloc, ex.cp, dtype=torch.bfloat16, device=gpu)
    g.body(xh)[:g.rows].view(b, g.p, ex.cp)[:, :, :ci] = x.bfloat16().to(gpu)
    y, partial, nrows = ex.forward_moments(xh, g)
    c = y.shape[1]
    mean, rstd = torch.full((c,), 7.0, device=gpu), torch.full((c,), 7.0, device=gpu)
    _call("rtts_bn_stats_from_partials", partial.data_ptr(), nrows, b, l, c, mean.data_ptr(), rstd.data_ptr(), None, None, None, None)
    torch.cuda.synchronize()
    st = _Stats(g.valid(y).reshape(b * l, c)[:, :co].cpu())
    if "full" in kind:
        assert (st.r >= 30).mean() >= 0.5, f"the input does not reach r >= 30 on half the channels: median {np.median(st.r):.1f}"
    em, er, ratio = st.check(mean[:co], rstd[:co], "conv epilogue")
    print(f"\n[bn statistics] path=conv-epilogue {kind} {b}x{l} {ci}->{co} r median {np.median(st.r):.1f} max {st.r.max():.1f}: rstd rel err {er:.2e} = "
          f"{ratio:.3f} of its bound, mean {em:.3f} of its (tol 1)")


# ================================================================== B / C. BatchNorm + activation + dropout, forward and backward
BN_SHAPES = [(2, 1, 8), (3, 5, 64), (2, 131, 320), (2, 64, 512)]
BN_LAYOUTS = [(0, "plain"), (2, "halo"), (2, "plain")]          # (halo of y, layout of z / dz)
SEED = 12345


class _BnCase:
    """Inputs and float64 reference of one BatchNorm + act + dropout case.  mean / rstd handed to the kernels are the float64
    statistics rounded to float32 (independent of the statistics kernels); the reference uses those rounded values."""

    def __init__(self, gpu, b, l, c, act, p, halo, seed=SEED, seed_dev=77):
        self.b, self.l, self.c, self.act, self.p, self.halo, self.seed = b, l, c, act, p, halo, seed
        self.m = b * l
        gen = torch.Generator().manual_seed(b * 1000 + l * 10 + c + act)
        y = (torch.randn(self.m, c, generator=gen) * 1.5 + 0.3).float()
        self.y64 = y.double().numpy()
        mean, var, rstd = R.bn_stats(self.y64)
        self.mean32, self.rstd32 = mean.astype(np.float32), rstd.astype(np.float32)
        self.gamma32 = (1 + 0.1 * torch.randn(c, generator=gen)).numpy()
        self.beta32 = (0.1 * torch.randn(c, generator=gen)).numpy()
        self.dz = torch.randn(self.m, c, generator=gen).bfloat16()
        self.keep = R.keep_mask(seed, seed_dev, p, R.bn_idx(b, l, halo, c))
        self.yh = _to_halo(y, b, l, halo, float("nan")).to(gpu)
        self.dev = {k: torch.from_numpy(v).to(gpu) for k, v in (("mean", self.mean32), ("rstd", self.rstd32), ("gamma", self.gamma32),
                                                                 ("beta", self.beta32))}
        self.seed_dev = None if seed_dev is None else torch.tensor([seed_dev], dtype=torch.int32, device=gpu)
        self.stat = [a.astype(np.float64) for a in (self.mean32, self.rstd32, self.gamma32, self.beta32)]

    def stat_ptrs(self):
        return [self.dev[k].data_ptr() for k in ("mean", "rstd", "gamma", "beta")]

    def unsure(self, pre):
        """ReLU elements whose gate float32 may decide the other way; must stay below 0.1 % of the case."""
        if self.act != 1:
            return np.zeros(pre.shape, dtype=bool)
        bad = np.abs(pre) < 1e-5 * (1 + np.abs(self.stat[3]))
        assert bad.mean() < 1e-3, f"{bad.sum()} of {bad.size} elements sit on the ReLU gate"
        return bad

    def forward(self, gpu, layout):
        """-> z (B*L, C) float64 of the kernel's bf16; asserts zeros outside the valid rows."""
        if layout == "halo":
            rows = LEAD + self.b * (self.l + 2 * self.halo) + TAIL
            zh = torch.full((rows, self.c), 7.0, dtype=torch.bfloat16, device=gpu)
            zargs = (1, LEAD, rows)
        else:
            zh = torch.full((self.m, self.c), 7.0, dtype=torch.bfloat16, device=gpu)
            zargs = (0, 0, self.m)
        _call("rtts_bn_act_fwd", self.yh.data_ptr(), *self.stat_ptrs(), self.act, self.p, self.seed, _ptr(self.seed_dev), self.b, self.l, self.halo,
              self.c, zh.data_ptr(), *zargs)
        torch.cuda.synchronize()
        if layout == "halo":
            z, rest = _split_halo(zh, self.b, self.l, self.halo, LEAD)
            assert bool((rest.float() == 0).all()), "z is not zero outside its valid rows"
            return _f64(z)
        return _f64(zh)

    def check_forward(self, z, tag):
        ref, pre = R.bn_act_fwd(self.y64, *self.stat, self.act, self.keep, self.p)
        ok = ~self.unsure(pre)
        err, tol = np.abs(z - ref), R.BF16_U * np.abs(ref) + 2e-6
        assert (z[~self.keep] == 0).all(), "a dropped element is not exactly zero"
        if self.p > 0 and self.m * self.c >= 64:
            assert 0 < (~self.keep).mean() < 2 * self.p + 0.2
        ratio = float((err / tol)[ok].max())
        print(f"\n[bn_act_fwd] {tag}: |z - z64| / (2^-8 |z64| + 2e-6) worst {ratio:.3f}, max abs err {err[ok].max():.2e} (tol 1)")
        assert ratio <= 1.0, (tag, ratio)

    def dz_dev(self, gpu, layout):
        if layout == "halo":
            return _to_halo(self.dz, self.b, self.l, self.halo, float("nan")).to(gpu), 1
        return self.dz.to(gpu), 0

    def dy_buffer(self, gpu, layout):
        lead, tail = (LEAD, TAIL) if layout == "halo" else (0, 0)
        rows = lead + self.b * (self.l + 2 * self.halo) + tail
        return torch.full((rows, self.c), 7.0, dtype=torch.bfloat16, device=gpu), lead, rows

    def grad_start(self, gpu):
        rs = np.random.RandomState(self.c)
        g0, b0 = (0.5 * rs.standard_normal(self.c)).astype(np.float32), (0.5 * rs.standard_normal(self.c)).astype(np.float32)
        return g0, b0, torch.from_numpy(g0).to(gpu), torch.from_numpy(b0).to(gpu)

    def backward(self, gpu, layout, split=False):
        """rtts_bn_act_bwd (or _sums + _apply(count = B*L)) -> dy buffer, its lead, dgamma, dbeta (device) and their starts."""
        dzd, dz_halo = self.dz_dev(gpu, layout)
        dyh, lead, rows = self.dy_buffer(gpu, layout)
        g0, b0, dg, db = self.grad_start(gpu)
        ws = _ws(gpu, self.c)
        head = (self.yh.data_ptr(), dzd.data_ptr(), dz_halo, *self.stat_ptrs(), self.act, self.p, self.seed, _ptr(self.seed_dev), self.b, self.l,
                self.halo, self.c)
        if split:
            sums = torch.full((2 * self.c + 1,), float("nan"), device=gpu)
            _call("rtts_bn_act_bwd_sums", *head, sums.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr())
            _call("rtts_bn_act_bwd_apply", *head, sums.data_ptr(), self.m, dyh.data_ptr(), lead, rows)
        else:
            _call("rtts_bn_act_bwd", *head, dyh.data_ptr(), lead, rows, dg.data_ptr(), db.data_ptr(), ws.data_ptr())
        torch.cuda.synchronize()
        return dyh, lead, dg, db, g0, b0

    def check_backward(self, dyh, lead, dg, db, g0, b0, tag, ref=None):
        dy, rest = _split_halo(dyh, self.b, self.l, self.halo, lead)
        assert bool((rest.float() == 0).all()), "dy is not zero outside its valid rows"
        ref = R.bn_act_bwd(self.y64, self.dz.double().numpy(), *self.stat, self.act, self.keep, self.p) if ref is None else ref
        ok = ~self.unsure(ref["pre"])
        err = np.abs(_f64(dy) - ref["dy"])
        tol = _dy_tol(ref, ref["dy"], self.stat, self.m)
        rdy = float((err / np.maximum(tol, 1e-300))[ok].max())
        want_b, want_g = b0 + ref["dbeta"], g0 + ref["dgamma"]
        tol_b = 2.0 ** -18 * np.abs(ref["g"]).sum(0) + U * np.abs(want_b)
        tol_g = 2.0 ** -18 * np.abs(ref["g"] * ref["yhat"]).sum(0) + U * np.abs(want_g)
        rb, rg = float((np.abs(_f64(db) - want_b) / tol_b).max()), float((np.abs(_f64(dg) - want_g) / tol_g).max())
        print(f"\n[bn_act_bwd] {tag}: worst error / bound  dy {rdy:.3f}  dgamma {rg:.3f}  dbeta {rb:.3f} (tol 1)")
        assert rdy <= 1.0 and rg <= 1.0 and rb <= 1.0, (tag, rdy, rg, rb)


def _dy_tol(ref, dy64, stat, m):
    """2^-8 |dy64| + 2e-5 max|dy64|, plus the float32 roundings of the three terms dy is the difference of:
    8 u |gamma rstd| (|g| + |sum g| / M + |yhat sum(g yhat)| / M).  With two rows per channel (B = 2, L = 1) yhat = +-1 and the exact dy
    is ZERO for every input, so max|dy64| is float64 noise and only this term describes what float32 can deliver; elsewhere it
    widens the bound by a few per cent (8 u = 4.8e-7 against 2e-5)."""
    mean, rstd, gamma, beta = stat
    terms = np.abs(gamma * rstd) * (np.abs(ref["g"]) + np.abs(ref["g"].sum(0)) / m + np.abs(ref["yhat"] * (ref["g"] * ref["yhat"]).sum(0)) / m)
    return R.BF16_U * np.abs(dy64) + 2e-5 * np.abs(dy64).max() + 8 * U * terms


def _bn_both(gpu, case, layout, tag):
    z = case.forward(gpu, layout)
    case.check_forward(z, tag)
    if case.halo and layout == "halo":
        assert np.array_equal(case.forward(gpu, "plain"), z), "plain-row z differs from the halo-row z"
    out = case.backward(gpu, layout)
    case.check_backward(*out, tag)
    # the data-parallel pair with the local count is the same arithmetic: bit for bit
    out2 = case.backward(gpu, layout, split=True)
    for a, b_, name in zip((out[0], out[2], out[3]), (out2[0], out2[2], out2[3]), ("dy", "dgamma", "dbeta")):
        assert torch.equal(a, b_), f"rtts_bn_act_bwd_sums + _apply differs from rtts_bn_act_bwd in {name}"
    if case.halo:
        # dz in the other layout: same numbers
        other = "plain" if layout == "halo" else "halo"
        dzd, dz_halo = case.dz_dev(gpu, other)
        dyh, lead, rows = case.dy_buffer(gpu, layout)
        g0, b0, dg, db = case.grad_start(gpu)
        _call("rtts_bn_act_bwd", case.yh.data_ptr(), dzd.data_ptr(), dz_halo, *case.stat_ptrs(), case.act, case.p, case.seed, _ptr(case.seed_dev), case.b,
              case.l, case.halo, case.c, dyh.data_ptr(), lead, rows, dg.data_ptr(), db.data_ptr(), _ws(gpu, case.c).data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(dyh, out[0]) and torch.equal(dg, out[2]) and torch.equal(db, out[3]), "dz layout changes the result"


@pytest.mark.parametrize("b,l,c", BN_SHAPES)
@pytest.mark.parametrize("halo,layout", BN_LAYOUTS)
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("act", [1, 2])
def test_bn_act_fwd_bwd_vs_float64(gpu, act, p, halo, layout, b, l, c):
    """rtts_bn_act_fwd, rtts_bn_act_bwd and rtts_bn_act_bwd_sums + rtts_bn_act_bwd_apply against float64 with the host-built mask."""
    _bn_both(gpu, _BnCase(gpu, b, l, c, act, p, halo), layout, f"act {act} p {p} {b}x{l}x{c} halo {halo} {layout}")


@pytest.mark.parametrize("seed,seed_dev", [(0xFFFFFFF0, 0x20), (SEED, None)])
def test_bn_act_seed_wrap_and_no_device_seed(gpu, seed, seed_dev):
    """seed + seed_dev[0] wraps modulo 2^32; seed_dev = NULL means the host seed alone."""
    _bn_both(gpu, _BnCase(gpu, 3, 5, 64, 2, 0.3, 2, seed=seed, seed_dev=seed_dev), "halo", f"seed {seed:#x} seed_dev {seed_dev}")


def test_bn_act_grid_stride(gpu):
    """More than 4096 * 256 groups of four elements: every thread of the capped grid takes a second element group."""
    b, l, c = 2, 4200, 512
    assert (LEAD + b * (l + 4) + TAIL) * c // 4 > 4096 * 256
    _bn_both(gpu, _BnCase(gpu, b, l, c, 2, 0.3, 2), "halo", f"grid-stride {b}x{l}x{c}")


@pytest.mark.parametrize("b,l,c", [(3, 5, 64), (3, 131, 320)])
@pytest.mark.parametrize("halo,layout", BN_LAYOUTS)
@pytest.mark.parametrize("act,p", [(1, 0.0), (2, 0.3), (1, 0.3)])
def test_bn_act_bwd_two_simulated_ranks(gpu, act, p, halo, layout, b, l, c):
    """Data-parallel backward without the second process: 2 + 1 samples, per-part sums (row count in slot 2C) added as an all-reduce
    would, rtts_bn_act_bwd_apply(count = 0) per part, against float64 BatchNorm backward over the WHOLE batch.  Each rank indexes its
    own y, so the dropout masks are per part."""
    whole = _BnCase(gpu, b, l, c, act, p, halo)
    parts, keeps = [], []
    for lo, hi in ((0, 2), (2, 3)):
        part = _BnCase.__new__(_BnCase)
        part.__dict__.update(whole.__dict__)
        part.b, part.m = hi - lo, (hi - lo) * l
        part.y64, part.dz = whole.y64[lo * l:hi * l], whole.dz[lo * l:hi * l]
        part.keep = R.keep_mask(SEED, 77, p, R.bn_idx(hi - lo, l, halo, c))
        part.yh = _to_halo(torch.from_numpy(part.y64).float(), hi - lo, l, halo, float("nan")).to(gpu)
        parts.append(part)
        keeps.append(part.keep)
    keep = np.concatenate(keeps)
    ref = R.bn_act_bwd(whole.y64, whole.dz.double().numpy(), *whole.stat, act, keep, p)
    total, state = torch.zeros(2 * c + 1, device=gpu), []
    g0, b0, dg, db = whole.grad_start(gpu)
    for part in parts:
        dzd, dz_halo = part.dz_dev(gpu, layout)
        head = (part.yh.data_ptr(), dzd.data_ptr(), dz_halo, *part.stat_ptrs(), act, p, SEED, _ptr(part.seed_dev), part.b, l, halo, c)
        sums = torch.full((2 * c + 1,), float("nan"), device=gpu)
        _call("rtts_bn_act_bwd_sums", *head, sums.data_ptr(), dg.data_ptr(), db.data_ptr(), _ws(gpu, c).data_ptr())
        sums[2 * c] = float(part.m)
        total += sums
        state.append((head, dzd))
    worst = 0.0
    for i, (part, (head, dzd)) in enumerate(zip(parts, state)):
        dyh, lead, rows = part.dy_buffer(gpu, layout)
        _call("rtts_bn_act_bwd_apply", *head, total.data_ptr(), 0, dyh.data_ptr(), lead, rows)
        torch.cuda.synchronize()
        dy, rest = _split_halo(dyh, part.b, l, halo, lead)
        assert bool((rest.float() == 0).all())
        sl = slice(0, 2 * l) if i == 0 else slice(2 * l, 3 * l)
        ok = ~whole.unsure(ref["pre"])[sl]
        tol = _dy_tol(ref, ref["dy"], whole.stat, whole.m)[sl]
        ratio = (np.abs(_f64(dy) - ref["dy"][sl]) / np.maximum(tol, 1e-300))[ok].max()
        worst = max(worst, float(ratio))
    # dgamma / dbeta: both parts accumulated into the same non-zero starting values
    want_b, want_g = b0 + ref["dbeta"], g0 + ref["dgamma"]
    tol_b = 2.0 ** -18 * np.abs(ref["g"]).sum(0) + 2 * U * (np.abs(b0) + np.abs(ref["g"]).sum(0))
    tol_g = 2.0 ** -18 * np.abs(ref["g"] * ref["yhat"]).sum(0) + 2 * U * (np.abs(g0) + np.abs(ref["g"] * ref["yhat"]).sum(0))
    rb, rg = float((np.abs(_f64(db) - want_b) / tol_b).max()), float((np.abs(_f64(dg) - want_g) / tol_g).max())
    print(f"\n[bn_act_bwd] two ranks act {act} p {p} {b}x{l}x{c} halo {halo} {layout}: worst error / bound  dy {worst:.3f}  dgamma {rg:.3f}  "
          f"dbeta {rb:.3f} (tol 1)")
    assert worst <= 1.0 and rb <= 1.0 and rg <= 1.0


# ================================================================== D. scaled positional encoding
PE_SHAPES = [(1, 1, 4), (3, 7, 8), (2, 131, 512), (4, 2100, 512)]
_pe = {}


def _pe_input(b, t, d):
    if (b, t, d) not in _pe:
        gen = torch.Generator().manual_seed(b * t + d)
        y = torch.randn(b * t, d, generator=gen).bfloat16()
        # |table| in [0.5, 1.5): a kept element never vanishes against y in float32, so the zero pattern of out - y is the mask
        table = torch.where(torch.rand(t, d, generator=gen) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(t, d, generator=gen))
        dy = torch.randn(b * t, d, generator=gen)
        _pe[b, t, d] = (y, table.float(), dy.float())
    return _pe[b, t, d]


@pytest.mark.parametrize("alpha", [1.0, -0.37, 0.0])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("b,t,d", PE_SHAPES)
def test_pe_add_and_dalpha_vs_float64(gpu, b, t, d, p, alpha):
    y, table, dy = _pe_input(b, t, d)
    seed, sdev = 0xFFFFFF00, 0x1A5                              # wraps
    keep = R.keep_mask(seed, sdev, p, R.pe_idx(t, d))
    a32 = float(np.float32(alpha))
    sd = torch.tensor([sdev], dtype=torch.int32, device=gpu)
    al = torch.tensor([a32], dtype=torch.float32, device=gpu)
    yd, td = y.to(gpu), table.to(gpu)
    out = torch.full((b * t + 1, d), 7.0, dtype=torch.float32, device=gpu)
    _call("rtts_pe_add", yd.data_ptr(), td.data_ptr(), al.data_ptr(), p, seed, sd.data_ptr(), t, b * t, d, out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out[b * t:] == 7.0).all()), "wrote behind the M rows"
    got = _f64(out[:b * t]).reshape(b, t, d)
    y64, t64 = y.double().numpy().reshape(b, t, d), table.double().numpy()
    ref = R.pe_add(y64, t64, a32, keep, p)
    tol = 4 * U * (np.abs(y64) + np.abs(a32 * t64)[None] * R.keep_scale(p))
    ratio = float((np.abs(got - ref) / np.maximum(tol, 1e-300)).max())
    if alpha != 0:
        moved = (got - y64) != 0
        for i in range(b):
            assert np.array_equal(moved[i], keep), f"sample {i}: the zero pattern of out - y is not the rebuilt mask"
    else:
        assert np.array_equal(got, y64)
    # dalpha accumulates into a non-zero value
    start = 0.75
    da = torch.tensor([start], dtype=torch.float32, device=gpu)
    ws = torch.full((512 + 1,), 7.0, device=gpu)
    dyd = dy.to(gpu)
    _call("rtts_pe_dalpha", dyd.data_ptr(), td.data_ptr(), p, seed, sd.data_ptr(), t, b * t, d, da.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    assert float(ws[512]) == 7.0
    want, mass = R.pe_dalpha(dy.double().numpy().reshape(b, t, d), t64, keep, p)
    delta = abs(float(da.cpu().double()) - (start + want))
    tol_a = 2.0 ** -18 * mass
    print(f"\n[pe_add] {b}x{t}x{d} p {p} alpha {alpha}: |out - ref| / bound {ratio:.3f};  [pe_dalpha] |delta| {delta:.2e} (tol {tol_a:.2e})")
    assert ratio <= 1.0
    assert delta <= tol_a, (delta, tol_a)


# ================================================================== E. relu + dropout in place
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("n", [8, 8 * 1000, 8 * (4096 * 256 + 3)])
def test_relu_drop_vs_float64(gpu, n, p):
    gen = torch.Generator().manual_seed(n % 1000)
    h = torch.randn(n, generator=gen)
    # negatives, both zeros, the smallest and the fullest mantissa (the keep-scales 1 and 2 of p = 0 and 0.5 are powers of two: the
    # scaled value is itself a bf16 number and any rounding of it at all, tie or not, is an error), tiny and large magnitudes
    special = torch.tensor([0.0, -0.0, -1.5, 1.0 + 2.0 ** -7, 1.9921875, 2.0 ** -100, -2.0 ** -120, 255.0])
    h[:8] = special
    h = h.bfloat16()
    seed, sdev = 99, 0xFFFFFFFF                               # wraps to 98
    keep = R.keep_mask(seed, sdev, p, np.arange(n, dtype=np.uint64))
    hd = torch.cat([h, torch.full((8,), -7.0, dtype=torch.bfloat16)]).to(gpu)
    sd = torch.tensor([-1], dtype=torch.int32, device=gpu)
    _call("rtts_relu_drop", hd.data_ptr(), p, seed, sd.data_ptr(), n)
    torch.cuda.synchronize()
    assert bool((hd[n:] == -7.0).all()), "wrote behind the n elements"
    got, h64 = _f64(hd[:n]), h.double().numpy()
    ref = R.relu_drop(h64, keep, p)
    err = np.abs(got - ref)
    assert (got[(~keep) | (h64 <= 0)] == 0).all(), "a dropped or negative element is not exactly zero"
    ratio = float((err / np.maximum(R.U9 * np.abs(ref), 1e-300))[ref != 0].max())
    print(f"\n[relu_drop] n {n} p {p}: |out - ref| / (2^-9 |ref|) worst {ratio:.3f} (tol 1), kept {keep.mean():.3f}")
    assert ratio <= 1.0
    if p == 0:
        assert torch.equal(hd[:n].cpu(), torch.relu(h.float()).bfloat16())
    else:
        assert abs(keep.mean() - 0.5) < (0.51 if n == 8 else 0.02)


# ================================================================== F. layout kernels (bit-exact)
def _ties(shape, gen):
    """float32 values of which every fourth sits exactly between two bf16 neighbours (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6):
    round-to-nearest-even is the only rounding that reproduces torch's .bfloat16() on them."""
    x = torch.randn(shape, generator=gen)
    flat = x.view(-1)
    k = torch.arange(0, flat.numel(), 4)
    odd = (k // 4) % 2
    flat[k] = torch.sign(flat[k] + 1e-9) * (1.0 + (1 + 2 * odd) * 2.0 ** -8) * 2.0 ** ((k // 8) % 5 - 2).float()
    return x


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("l", [1, 131])
@pytest.mark.parametrize("halo,lead,tail", [(0, 0, 0), (2, 0, 0), (2, 8, 11), (0, 3, 2)])
@pytest.mark.parametrize("c_src,ld,c", [(80, 96, 128), (64, 64, 64), (8, 8, 8)])
@pytest.mark.parametrize("src_f32", [1, 0])
def test_to_halo_bit_exact(gpu, src_f32, c_src, ld, c, halo, lead, tail, l):
    """fp32 and bf16 sources, C_src < C (zero padding), ld_src > C_src, a time-sliced view (batch stride over L + 3 rows)."""
    b = 3
    gen = torch.Generator().manual_seed(l + c + halo)
    data = _ties((b, l, c_src), gen)
    if not src_f32:
        data = data.bfloat16()
    src = torch.full((b, l + 3, ld), float("nan"), dtype=data.dtype)        # what lies between the rows and samples is never read
    src[:, :l, :c_src] = data
    rows = lead + b * (l + 2 * halo) + tail
    dst = torch.full((rows + 1, c), 7.0, dtype=torch.bfloat16, device=gpu)
    srcd = src.to(gpu)
    _call("rtts_to_halo", srcd.data_ptr(), ld, (l + 3) * ld, c_src, src_f32, b, l, halo, c, dst.data_ptr(), lead, rows)
    torch.cuda.synchronize()
    assert bool((dst[rows:] == 7.0).all()), "wrote behind the rows it was given"
    want = torch.zeros(rows, c, dtype=torch.bfloat16)
    want[torch.from_numpy(_valid_rows(b, l, halo, lead)), :c_src] = data.reshape(b * l, c_src).bfloat16()
    assert torch.equal(_bits(dst[:rows].cpu()), _bits(want))
    if c_src == c and ld == c:
        # contiguous source: src_batch_stride 0 means L * ld_src
        srcc = data.contiguous().to(gpu)
        dst2 = torch.full((rows, c), 7.0, dtype=torch.bfloat16, device=gpu)
        _call("rtts_to_halo", srcc.data_ptr(), ld, 0, c_src, src_f32, b, l, halo, c, dst2.data_ptr(), lead, rows)
        torch.cuda.synchronize()
        assert torch.equal(_bits(dst2.cpu()), _bits(want))


PERM_SHAPES = [(3, 5, 8), (80, 512, 512), (512, 80, 128), (128, 128, 128)]


def _perm_want(w, cp):
    co, ci, _ = w.shape
    want = torch.zeros(co, 5, cp, dtype=torch.bfloat16)
    want[:, :, :ci] = w.permute(0, 2, 1).bfloat16()
    return want


def _jobs(items):
    from reformer_tts_amd import _lib
    jobs = (_lib.ConvPermJob * len(items))()
    for j, (src, dst, co, ci, cp) in zip(jobs, items):
        j.w, j.wp, j.Co, j.Ci, j.CP = src.data_ptr(), dst.data_ptr(), co, ci, cp
    return jobs


@pytest.mark.parametrize("co,ci,cp", PERM_SHAPES)
def test_conv_w_perm_bit_exact(gpu, co, ci, cp):
    w = _ties((co, ci, 5), torch.Generator().manual_seed(co + ci))
    wd = w.to(gpu)
    wp = torch.full((co * 5 * cp + 8,), 7.0, dtype=torch.bfloat16, device=gpu)
    _call("rtts_conv_w_perm", wd.data_ptr(), co, ci, cp, wp.data_ptr())
    torch.cuda.synchronize()
    want = _perm_want(w, cp)
    assert bool((wp[co * 5 * cp:] == 7.0).all())
    assert torch.equal(_bits(wp[:co * 5 * cp].cpu()), _bits(want.view(-1)))
    # the grouped form with one job: the same bits
    wp1 = torch.full((co * 5 * cp + 8,), 7.0, dtype=torch.bfloat16, device=gpu)
    _call("rtts_conv_w_perm_grouped", _jobs([(wd, wp1, co, ci, cp)]), 1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(wp1.cpu()), _bits(wp.cpu()))


GROUP = [(3, 5, 8), (80, 512, 512), (512, 80, 128), (128, 128, 128), (1, 1, 8), (7, 130, 256), (64, 64, 64), (5, 9, 16)]


def test_conv_w_perm_grouped_bit_identical_to_single_launches(gpu):
    gen = torch.Generator().manual_seed(8)
    ws = [_ties((co, ci, 5), gen).to(gpu) for co, ci, cp in GROUP]
    single = [torch.full((co * 5 * cp + 8,), 7.0, dtype=torch.bfloat16, device=gpu) for co, ci, cp in GROUP]
    grouped = [torch.full((co * 5 * cp + 8,), 7.0, dtype=torch.bfloat16, device=gpu) for co, ci, cp in GROUP]
    for w, dst, (co, ci, cp) in zip(ws, single, GROUP):
        _call("rtts_conv_w_perm", w.data_ptr(), co, ci, cp, dst.data_ptr())
    _call("rtts_conv_w_perm_grouped", _jobs([(w, dst, *s) for w, dst, s in zip(ws, grouped, GROUP)]), len(GROUP))
    torch.cuda.synchronize()
    for w, a, b_, (co, ci, cp) in zip(ws, single, grouped, GROUP):
        assert torch.equal(_bits(a.cpu()), _bits(b_.cpu())), (co, ci, cp)
        assert torch.equal(_bits(a[:co * 5 * cp].cpu()), _bits(_perm_want(w.cpu(), cp).view(-1))), (co, ci, cp)


def _dw_case(gpu, shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for co, ci, cp in shapes:
        dwp = torch.full((co, 5, cp), float("nan"))                         # the padded channels are never read
        dwp[:, :, :ci] = torch.randn(co, 5, ci, generator=gen)
        before = torch.randn(co, ci, 5, generator=gen)
        dw = torch.cat([before.view(-1), torch.full((8,), 7.0)]).to(gpu)
        want = before + dwp[:, :, :ci].permute(0, 2, 1)                     # one float32 addition per element: exact agreement
        out.append((dwp.to(gpu), dw, want, (co, ci, cp)))
    return out


@pytest.mark.parametrize("co,ci,cp", PERM_SHAPES)
def test_conv_dw_unperm_bit_exact(gpu, co, ci, cp):
    (dwp, dw, want, _), = _dw_case(gpu, [(co, ci, cp)], co)
    (dwp1, dw1, _, _), = _dw_case(gpu, [(co, ci, cp)], co)
    _call("rtts_conv_dw_unperm", dwp.data_ptr(), co, ci, cp, dw.data_ptr())
    _call("rtts_conv_dw_unperm_grouped", _jobs([(dwp1, dw1, co, ci, cp)]), 1)
    torch.cuda.synchronize()
    for got in (dw, dw1):
        assert bool((got[co * ci * 5:] == 7.0).all())
        assert torch.equal(_bits(got[:co * ci * 5].cpu()), _bits(want.view(-1)))


def test_conv_dw_unperm_grouped_bit_identical_to_single_launches(gpu):
    cases = _dw_case(gpu, GROUP, 5)
    _call("rtts_conv_dw_unperm_grouped", _jobs([(dwp, dw, *s) for dwp, dw, _, s in cases]), len(cases))
    torch.cuda.synchronize()
    for dwp, dw, want, (co, ci, cp) in cases:
        assert bool((dw[co * ci * 5:] == 7.0).all()), (co, ci, cp)
        assert torch.equal(_bits(dw[:co * ci * 5].cpu()), _bits(want.view(-1))), (co, ci, cp)


# ================================================================== G. rejections
@pytest.mark.parametrize("bad_p", [1.0, -0.1, 1.5, float("nan")])
def test_backward_entry_points_reject_bad_drop_p(gpu, bad_p):
    """drop_p outside [0, 1) is an RttsError naming the argument, raised before any launch: 1 / (1 - p) would be infinite (p = 1) or the
    threshold meaningless inside the kernel.  Every output keeps its prefill."""
    from reformer_tts_amd._lib import RttsError
    case = _BnCase(gpu, 3, 5, 64, 2, 0.0, 2)
    dzd, dz_halo = case.dz_dev(gpu, "halo")
    dyh, lead, rows = case.dy_buffer(gpu, "halo")
    g0, b0, dg, db = case.grad_start(gpu)
    sums = torch.full((2 * case.c + 1,), 7.0, device=gpu)
    ws = torch.full(((2 * PBLOCKS + 2) * case.c + 1,), 7.0, device=gpu)
    head = (case.yh.data_ptr(), dzd.data_ptr(), dz_halo, *case.stat_ptrs(), 2, bad_p, SEED, _ptr(case.seed_dev), case.b, case.l, case.halo, case.c)
    calls = {"rtts_bn_act_bwd": (*head, dyh.data_ptr(), lead, rows, dg.data_ptr(), db.data_ptr(), ws.data_ptr()),
             "rtts_bn_act_bwd_sums": (*head, sums.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr()),
             "rtts_bn_act_bwd_apply": (*head, sums.data_ptr(), case.m, dyh.data_ptr(), lead, rows)}
    y, table, dy = _pe_input(3, 7, 8)
    td, dyd = table.to(gpu), dy.to(gpu)
    da, pws = torch.tensor([0.75], device=gpu), torch.full((512,), 7.0, device=gpu)
    calls["rtts_pe_dalpha"] = (dyd.data_ptr(), td.data_ptr(), bad_p, SEED, None, 7, 21, 8, da.data_ptr(), pws.data_ptr())
    for name, args in calls.items():
        with pytest.raises(RttsError, match=rf"{name}: .*drop_p"):
            _call(name, *args)
    torch.cuda.synchronize()
    assert bool((dyh == 7.0).all()) and bool((sums == 7.0).all()) and bool((ws == 7.0).all()) and bool((pws == 7.0).all())
    assert float(da) == 0.75 and np.array_equal(_f64(dg), g0.astype(np.float64)) and np.array_equal(_f64(db), b0.astype(np.float64))


@pytest.mark.parametrize("bad_d", [0, -4])
def test_pe_dalpha_rejects_bad_width(gpu, bad_d):
    from reformer_tts_amd._lib import RttsError
    y, table, dy = _pe_input(3, 7, 8)
    td, dyd = table.to(gpu), dy.to(gpu)
    da, pws = torch.tensor([0.75], device=gpu), torch.full((512,), 7.0, device=gpu)
    with pytest.raises(RttsError, match=r"rtts_pe_dalpha: d must"):
        _call("rtts_pe_dalpha", dyd.data_ptr(), td.data_ptr(), 0.0, SEED, None, 7, 21, bad_d, da.data_ptr(), pws.data_ptr())
    torch.cuda.synchronize()
    assert float(da) == 0.75 and bool((pws == 7.0).all())
