"""The convolution form of rtts_gemm_nt's main loop (csrc/gemm_nt.hip, MODE 3): the input rows [m0 - 2, m0 + BM + 2) of every
channel block stay in LDS as one image each, and the five taps read them at five row shifts; K keeps the plain loop's
(tap-major) order, so the two loops agree bit for bit.  Everything here goes through the C ABI (rtts_conv1d_k5 /
rtts_conv1d_k5_moments) on halo rows laid out by this file, so that C_in = 64 (one channel block: fewer images than ring
stages), two blocks, eight blocks (the LDS limit of the 4-wave tiles) and every tile family of gn_pick are reachable (the
256 x 256 tile, and channel counts whose images do not fit LDS, run the plain loop: the checks are the same):

  family     reached by (M, N)                               here
  128 x 64   small problems, M % 128 == 0                    the four basic shapes, M rounded up to 128
  96 x 64    small problems, M % 96 == 0, M % 128 != 0       M rounded up to 96
  192 x 128  M % 192 == 0, (M / 192) (N / 128) >= 192        M = 9216, N = 512
  256 x 128  (M / 256) (N / 128) >= 192, M % 192 != 0        M = 12544, N = 512 (the postnet's own shape)
  256 x 256  (M / 256) (N / 256) % 256 == 0                  M = 32768, N = 512

N is C_out for the forward and C_in for the transposed product, so the large families get one shape per direction (64 -> 512
and 512 -> 64; both directions are checked on both, whichever family the other one lands on).  Tolerance: rel-L2 <= 1e-5
against float64 on the same bf16-rounded operands, as tests/test_model_hip.py::test_conv1d_k5_implicit_gemm_vs_float64 --
the outputs are unrounded fp32, what is left is the fp32 accumulation over K = 5 C_in <= 2560 terms.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LEAD = 8          # rows in front of halo row 0 (the kernel may read 2 of them)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")

# (B, L, C_in, C_out, M rounded up to, (BM, WM, BM == BN == 256) of the forward's family or None, of the transposed product's)
BASIC = [
    (1, 5, 64, 64, 128, (128, 2, False), (128, 2, False)),
    (2, 37, 128, 64, 128, (128, 2, False), (128, 2, False)),
    (3, 131, 64, 128, 128, (128, 2, False), (128, 2, False)),
    (2, 260, 512, 80, 128, (128, 2, False), (128, 2, False)),
]
# one shape per family whose rows B (L + 4) end 3 .. 5 rows behind a tile boundary: the last tile that carries data holds 1 .. 3
# data rows, and the rows of the sequence in front of it sit in its halo
CROSSING = [
    (9, 25, 64, 64, 128, (128, 2, False), (128, 2, False)),          # 261 = 2 * 128 + 5
    (1, 193, 128, 64, 96, (96, 2, False), (96, 2, False)),           # 197 = 2 * 96 + 5
    (3, 131, 64, 128, 96, (96, 2, False), (96, 2, False)),           # 405 rows in 5 tiles of 96, one channel block
    (9, 999, 64, 512, 192, (192, 4, False), None),                   # 9027 = 47 * 192 + 3
    (9, 999, 512, 64, 192, None, (192, 4, False)),
    (3, 4093, 64, 512, 256, (256, 4, False), None),                  # 12291 = 48 * 256 + 3, M = 12544
    (3, 4093, 512, 64, 256, None, (256, 4, False)),
    (35, 925, 64, 512, 256, (256, 4, True), None),                   # 32515 = 127 * 256 + 3, M = 32768
    (35, 925, 512, 64, 256, None, (256, 4, True)),
]


def _pad64(c):
    return -(-c // 64) * 64


def _family_is(lib, m, n, fam):
    bm, wm, sq = fam
    return lib.rtts_gemm_nt_partial_rows(m, n) == m // bm * wm and (lib.rtts_gemm_nt_gate_words(m, n) == 0) == sq


class _Case:
    """One convolution on halo rows: operands on the GPU (bf16), the kernel's outputs, and the float64 references."""

    def __init__(self, gpu, b, l, ci, co, round_to, fill_halo, mode=20):
        """mode: rtts_debug_set_gemm_mode -- 20 the library's pick, 21 the plain loop, 22 the convolution form where it fits"""
        from reformer_tts_amd import _lib
        self.b, self.l, self.ci, self.co = b, l, ci, co
        self.cp, self.cop = _pad64(ci), _pad64(co)
        self.p = l + 4
        self.rows = b * self.p
        self.m = -(-self.rows // round_to) * round_to
        g = torch.Generator(device="cpu").manual_seed(1000 * b + l + ci + co)
        s = torch.cuda.current_stream().cuda_stream
        w = torch.randn(co, ci, 5, generator=g) / (5 * ci) ** 0.5
        self.w_bf = w.bfloat16()
        wp = torch.zeros(self.cop, 5 * self.cp, dtype=torch.bfloat16, device=gpu)
        wdev = w.to(gpu)
        _lib.call("rtts_conv_w_perm", wdev.data_ptr(), co, ci, self.cp, wp.data_ptr(), s)

        def rows_of(c, cpad, scale):
            """(LEAD + m + LEAD, cpad) bf16: data in the valid rows and channels; halo / padding rows zero, or data too
            (fill_halo); the rows the kernel must never read (more than 2 outside [0, m)) are NaN."""
            full = (torch.randn(self.m + 2 * LEAD, cpad, generator=g) * scale).bfloat16()
            full[:, c:] = 0
            if not fill_halo:
                body = torch.zeros(self.m, cpad, dtype=torch.bfloat16)
                v = body[:self.rows].view(b, self.p, cpad)[:, 2:2 + l]
                v.copy_(full[LEAD:LEAD + self.rows].view(b, self.p, cpad)[:, 2:2 + l])
                full.zero_()
                full[LEAD:LEAD + self.m] = body
            full[:LEAD - 2] = float("nan")
            full[LEAD + self.m + 2:] = float("nan")
            return full

        self.x = rows_of(ci, self.cp, 1.0)
        self.dy = rows_of(co, self.cop, 0.125)
        xd, dyd = self.x.to(gpu), self.dy.to(gpu)
        self.xd, self.wp = xd, wp
        self.y = torch.full((self.m, self.cop), float("nan"), dtype=torch.float32, device=gpu)
        self.dx = torch.full((self.m, self.cp), float("nan"), dtype=torch.float32, device=gpu)
        _lib.call("rtts_debug_set_gemm_mode", mode)
        try:
            _lib.call("rtts_conv1d_k5", xd[LEAD:].data_ptr(), self.cp, wp.data_ptr(), 5 * self.cp, 0, self.m, self.cop, self.cp, self.y.data_ptr(),
                      self.cop, None, 1, s)
            _lib.call("rtts_conv1d_k5", dyd[LEAD:].data_ptr(), self.cop, wp.data_ptr(), 5 * self.cp, 1, self.m, self.cp, self.cop,
                      self.dx.data_ptr(), self.cp, None, 1, s)
            torch.cuda.synchronize()
        finally:
            _lib.call("rtts_debug_set_gemm_mode", 20)

    def valid(self, t):
        """(B, L, C) view of the rows that carry data of an (m, C) array."""
        return t[:self.rows].view(self.b, self.p, -1)[:, 2:2 + self.l]

    def check_vs_conv1d(self):
        """zero halo: F.conv1d / its transpose per sequence, float64, the same bf16-rounded operands"""
        w64 = self.w_bf.double()
        x64 = self.valid(self.x[LEAD:LEAD + self.m])[..., :self.ci].double().transpose(1, 2)
        dy64 = self.valid(self.dy[LEAD:LEAD + self.m])[..., :self.co].double().transpose(1, 2)
        y64 = F.conv1d(x64, w64, None, padding=2).transpose(1, 2)
        dx64 = F.conv_transpose1d(dy64, w64, None, padding=2).transpose(1, 2)
        y, dx = self.y.cpu(), self.dx.cpu()
        e_y = float((self.valid(y)[..., :self.co].double() - y64).norm() / y64.norm())
        e_dx = float((self.valid(dx)[..., :self.ci].double() - dx64).norm() / dx64.norm())
        print(f"\n[conv taps B={self.b} L={self.l} {self.ci}->{self.co} M={self.m}] rel-L2 vs float64 F.conv1d: y {e_y:.2e}, dx {e_dx:.2e} (tol 1e-5)")
        assert e_y <= 1e-5 and e_dx <= 1e-5
        if self.cop > self.co:
            assert float(y[:, self.co:].abs().max()) == 0.0          # padded output channels: zero weight rows
        if self.cp > self.ci:
            assert float(dx[:, self.ci:].abs().max()) == 0.0

    def check_all_rows(self):
        """halo rows hold data: EVERY output row m -- the real tokens among them -- is the float64 convolution over exactly
        the row values m - 2 .. m + 2 of the array, across sequence and tile boundaries (one long sequence, no padding)"""
        w64 = self.w_bf.double()
        xs = self.x[LEAD - 2:LEAD + self.m + 2, :self.ci].double().t().unsqueeze(0)
        dys = self.dy[LEAD - 2:LEAD + self.m + 2, :self.co].double().t().unsqueeze(0)
        y64 = F.conv1d(xs, w64, None, padding=0)[0].t().contiguous()
        dx64 = F.conv_transpose1d(dys, w64, None, padding=4)[0].t().contiguous()
        y, dx = self.y.cpu(), self.dx.cpu()
        assert y64.shape[0] == self.m and dx64.shape[0] == self.m
        e_y = float((y[:, :self.co].double() - y64).norm() / y64.norm())
        e_dx = float((dx[:, :self.ci].double() - dx64).norm() / dx64.norm())
        e_yv = float((self.valid(y)[..., :self.co].double() - self.valid(y64)).norm() / self.valid(y64).norm())
        e_dxv = float((self.valid(dx)[..., :self.ci].double() - self.valid(dx64)).norm() / self.valid(dx64).norm())
        print(f"\n[conv taps, data in the halo B={self.b} L={self.l} {self.ci}->{self.co} M={self.m}] rel-L2 vs float64: all rows y {e_y:.2e}, "
              f"dx {e_dx:.2e}; token rows y {e_yv:.2e}, dx {e_dxv:.2e} (tol 1e-5)")
        assert max(e_y, e_dx, e_yv, e_dxv) <= 1e-5


def _check_families(b, l, ci, co, round_to, fam_f, fam_t):
    """the shape reaches the tile family it is listed for (gn_pick is the library's; a changed pick must not hollow the list out)"""
    from reformer_tts_amd import _lib
    lib = _lib.load()
    m = -(-(b * (l + 4)) // round_to) * round_to
    if fam_f is not None:
        assert _family_is(lib, m, _pad64(co), fam_f), (m, _pad64(co), fam_f)
    if fam_t is not None:
        assert _family_is(lib, m, _pad64(ci), fam_t), (m, _pad64(ci), fam_t)


@pytest.mark.parametrize("b,l,ci,co,round_to,fam_f,fam_t", BASIC + CROSSING)
def test_conv_taps_forward_and_transposed_vs_float64(gpu, b, l, ci, co, round_to, fam_f, fam_t):
    _check_families(b, l, ci, co, round_to, fam_f, fam_t)
    _Case(gpu, b, l, ci, co, round_to, fill_halo=False).check_vs_conv1d()


@pytest.mark.parametrize("b,l,ci,co,round_to,fam_f,fam_t", BASIC + CROSSING)
def test_conv_taps_halo_rows_with_data(gpu, b, l, ci, co, round_to, fam_f, fam_t):
    _Case(gpu, b, l, ci, co, round_to, fill_halo=True).check_all_rows()


@pytest.mark.parametrize("b,l,ci,co,round_to,fam_f,fam_t", BASIC + CROSSING)
def test_conv_taps_both_loops_agree_bit_for_bit(gpu, b, l, ci, co, round_to, fam_f, fam_t):
    """the convolution form sums over K in the plain loop's order: forward and transposed product are equal bit for bit"""
    plain = _Case(gpu, b, l, ci, co, round_to, fill_halo=True, mode=21)
    form = _Case(gpu, b, l, ci, co, round_to, fill_halo=True, mode=22)
    assert torch.equal(form.y, plain.y) and torch.equal(form.dx, plain.dx)
    assert bool(torch.isfinite(form.y).all()) and bool(torch.isfinite(form.dx).all())


@pytest.mark.parametrize("b,l,ci,co", [(3, 200, 128, 128), (2, 131, 512, 512)])
def test_conv_taps_moments_epilogue_bit_identical(gpu, b, l, ci, co):
    """rtts_conv1d_k5_moments returns the y of rtts_conv1d_k5, bit for bit, and the sums of y and y^2 over the token rows"""
    from reformer_tts_amd import _lib
    c = _Case(gpu, b, l, ci, co, 256, fill_halo=True)
    lib = _lib.load()
    nrows = lib.rtts_gemm_nt_partial_rows(c.m, c.cop)
    assert nrows > 0
    y = torch.full_like(c.y, float("nan"))
    partial = torch.full((nrows, 2 * c.cop), float("nan"), dtype=torch.float32, device=gpu)
    _lib.call("rtts_conv1d_k5_moments", c.xd[LEAD:].data_ptr(), c.cp, c.wp.data_ptr(), 5 * c.cp, c.m, c.cop, c.cp, y.data_ptr(), c.cop,
              b, l, 2, partial.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(y, c.y)
    yv = c.valid(c.y).double().reshape(-1, c.cop)
    sums = partial.double().sum(0)
    # fp32 sums of n <= 600 values of O(1): |error| <= n eps max|partial sum| ~ 600 * 6e-8 * 30 ~ 1e-3
    torch.testing.assert_close(sums[:c.cop], yv.sum(0), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(sums[c.cop:], (yv * yv).sum(0), rtol=1e-4, atol=1e-3)
