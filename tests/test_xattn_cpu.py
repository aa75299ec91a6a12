"""The float64 cross-attention oracle of tests/xattn_ref.py checked without a GPU: its forward against nn.MultiheadAttention, its
analytic gradients against float64 autograd (with and without an explicit dropout mask), the dropout mask twin, and the error
bounds -- the fp32 / bf16 model of the kernels' data flow must stay inside every bound on every input kind and chunk count that
tests/test_xattn_hip.py uses, and each of its seven deliberate defects must break one."""
import functools

import numpy as np
import pytest
import torch

import xattn_ref as X

# (T_k, kvalid pattern): the key counts of the GPU test's shape matrix -- 1, 1, 3, 5, 4, 9, 15 and 8 chunks
TK_PATTERNS = [(128, "ragged"), (256, "alternating"), (384, "first"), (640, "middle"), (1024, "last"), (1152, "one"),
               (1920, "ragged"), (2048, "none")]
DROPS = (None, (0.5, 77, 3), (0.1, 77, None))


def _rel(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


def _case(kind, nb, nh, tq, tk, pattern, drop, seed=None):
    q, k, v, do = X.make_inputs(kind, nb, nh, tq, tk, seed=tk + tq if seed is None else seed)
    valid = X.make_valid(pattern, nb, tk)
    keep = None if drop is None else X.keep_scales(*drop, nb * nh, tq, tk).view(nb, nh, tq, tk)
    return (q, k, v, do), valid, keep


@pytest.mark.parametrize("tk,pattern", [(128, "ragged"), (384, "middle"), (1920, "alternating")])
def test_reference_forward_equals_multihead_attention(tk, pattern):
    """``reference`` o == nn.MultiheadAttention (identity projections, key_padding_mask) in float64, to 1e-12 relative."""
    nb, nh, tq = 2, 3, 128
    (q, k, v, do), valid, _ = _case("plain", nb, nh, tq, tk, pattern, None)
    e = nh * X.DH
    mha = torch.nn.MultiheadAttention(e, nh, bias=False, batch_first=True).double().train()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(e, dtype=torch.float64).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(e, dtype=torch.float64))
    flat = lambda x: x.double().transpose(1, 2).reshape(nb, -1, e)
    want, _ = mha(flat(q), flat(k), flat(v), key_padding_mask=~valid, need_weights=True)
    got = flat(X.reference(q, k, v, do, valid)["o"])
    err = _rel(got, want.detach())
    print(f"\n[reference] forward vs nn.MultiheadAttention, {tk} keys ({pattern}): rel {err:.2e} (tol 1e-12)")
    assert err <= 1e-12


@pytest.mark.parametrize("drop", [None, (0.5, 123, 4)])
@pytest.mark.parametrize("kind,tk,pattern", [("plain", 256, "ragged"), ("peaked", 640, "first"), ("offset+", 1152, "alternating")])
def test_reference_gradients_equal_autograd(kind, tk, pattern, drop):
    """The analytic dQ, dK, dV (and lse, delta) == float64 autograd through softmax(mask(q k^T / 8)) o keep @ v, to 1e-10; with
    ``keep`` given the mask is the same explicit one, and lse is the one of the run without dropout, bit for bit."""
    nb, nh, tq = 2, 2, 128
    (q, k, v, do), valid, keep = _case(kind, nb, nh, tq, tk, pattern, drop)
    ref = X.reference(q, k, v, do, valid, keep)
    qr, kr, vr = (x.double().requires_grad_() for x in (q, k, v))
    s = (qr @ kr.transpose(-1, -2) / 8.0).masked_fill(~valid.view(nb, 1, 1, tk), float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = (p if keep is None else p * keep) @ vr
    o.backward(do.double())
    errs = dict(o=_rel(ref["o"], o.detach()), lse=_rel(ref["lse"], torch.logsumexp(s.detach(), -1)),
                delta=_rel(ref["delta"], (o.detach() * do.double()).sum(-1)), dq=_rel(ref["dq"], qr.grad), dk=_rel(ref["dk"], kr.grad),
                dv=_rel(ref["dv"], vr.grad))
    print(f"\n[reference] gradients vs autograd, {kind} {tk} keys ({pattern}), dropout {drop}: "
          + " ".join(f"{n} {e:.1e}" for n, e in errs.items()) + " (tol 1e-10)")
    assert max(errs.values()) <= 1e-10
    if drop is not None:
        assert torch.equal(ref["lse"], X.reference(q, k, v, do, valid)["lse"])
        assert not torch.equal(ref["o"], X.reference(q, k, v, do, valid)["o"])
    pad = ~valid.view(nb, 1, tk, 1).expand(nb, nh, tk, X.DH)
    for n in ("dk", "dv", "b_dk", "b_dv"):                        # padded keys: gradient and bound exactly 0
        assert float(ref[n][pad].abs().max()) == 0.0, n


@functools.lru_cache(maxsize=None)
def _model_ratios(kind, tk, pattern, drop, defect=None):
    nb, nh, tq = 2, 1, 256
    (q, k, v, do), valid, keep = _case(kind, nb, nh, tq, tk, pattern, drop)
    ref = X.reference(q, k, v, do, valid, keep)
    got = X.kernel_model(q, k, v, do, valid, drop, defect)
    r = X.ratios(got, ref)
    r["lse"] = X.lse_ratio(got["lse"], ref)
    return r


@pytest.mark.parametrize("kind", X.KINDS)
def test_kernel_model_stays_within_every_bound(kind):
    """Without a defect the fp32 / bf16 model of the kernels is inside every bound (ratio <= 1) on every input kind, key count,
    kvalid pattern and dropout rate of the GPU test: the inputs do not push the REFERENCE side of that comparison over its own
    bound.  (The model's lse needs c of about 2 in c 2^-24 (max_j sum |q k| / 8 + |lse| + 1).)"""
    worst = dict(o=0.0, dq=0.0, dk=0.0, dv=0.0, lse=0.0)
    for tk, pattern in TK_PATTERNS:
        for drop in DROPS:
            r = _model_ratios(kind, tk, pattern, drop)
            worst = {n: max(worst[n], r[n]) for n in worst}
            assert max(r[n] for n in ("o", "dq", "dk", "dv")) <= 1.0, (tk, pattern, drop, r)
    print(f"\n[model] {kind}: worst |model - float64| / bound over {len(TK_PATTERNS) * len(DROPS)} cases: "
          + " ".join(f"{n} {x:.3f}" for n, x in worst.items()))
    assert worst["lse"] <= 4.0


@pytest.mark.parametrize("tk", [384, 1920])
@pytest.mark.parametrize("defect", X.DEFECTS)
def test_each_defect_breaks_a_bound(defect, tk):
    """Each deliberate error of ``kernel_model`` must FAIL at least one bound at 3 and at 15 key chunks (peaked inputs, ragged
    padding, dropout 0.5 -- the same case passes without the defect): a bound that let one through would let the kernel through."""
    clean = _model_ratios("peaked", tk, "ragged", (0.5, 77, 3))
    r = _model_ratios("peaked", tk, "ragged", (0.5, 77, 3), defect)
    broken = [n for n in ("o", "dq", "dk", "dv") if not r[n] <= 1.0]
    print(f"\n[defect {defect}] {tk} keys: " + " ".join(f"{n} {x:.3g}" for n, x in r.items()) + f" -> breaks {broken}")
    assert max(clean[n] for n in ("o", "dq", "dk", "dv")) <= 1.0
    assert broken, f"defect ({defect}) passes every bound at {tk} keys: {r}"


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_twin_keeps_the_right_fraction_and_seeds_do_not_alias(p):
    """The kept fraction is within 5e-3 of 1 - p; the masks of two seeds 0x9E3779B1 apart (the hash's index multiplier) are not
    shifted copies of one another: at every shift they agree as often as independent masks do, p^2 + (1 - p)^2."""
    bh, tq, tk = 4, 256, 512
    m0 = X.keep_scales(p, 1234, None, bh, tq, tk).reshape(-1) > 0
    m1 = X.keep_scales(p, 1234, 0x9E3779B1, bh, tq, tk).reshape(-1) > 0
    frac = float(m0.double().mean())
    assert abs(frac - (1 - p)) <= 5e-3 and abs(float(m1.double().mean()) - (1 - p)) <= 5e-3
    assert set(np.unique(X.keep_scales(p, 1234, None, 1, 128, 128).numpy())) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    assert torch.equal(X.keep_scales(p, 1234, 5, 1, 128, 128), X.keep_scales(p, 1239, None, 1, 128, 128))      # seed + *seed_dev
    indep = p * p + (1 - p) * (1 - p)
    n = m0.numel()
    for shift in range(-8, 9):
        a, b = (m0[shift:], m1[:n - shift]) if shift >= 0 else (m0[:n + shift], m1[-shift:])
        agree = float((a == b).double().mean())
        assert abs(agree - indep) <= 1e-2, (shift, agree)
