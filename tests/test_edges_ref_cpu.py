"""tests/edges_ref.py against torch in float64, on the CPU: the float64 references that tests/test_edges_hip.py and
tests/test_optim_hip.py hold the kernels to must themselves be right.  BatchNorm forward/backward with a fixed dropout mask against
torch.autograd, the running statistics against F.batch_norm, AdamW and the clip coefficient against oracle/optim_ref.py."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edges_ref as R
from oracle import optim_ref
from oracle.synth import drop_hash


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_bn_act_reference_vs_autograd(act, p):
    rs = np.random.RandomState(act * 7 + int(p * 10))
    b, l, c, halo = 3, 17, 12, 2
    m = b * l
    y = rs.standard_normal((m, c)) * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * rs.standard_normal(c), 0.1 * rs.standard_normal(c)
    dz = rs.standard_normal((m, c))
    keep = R.keep_mask(123, 77, p, R.bn_idx(b, l, halo, c))
    mean, var, rstd = R.bn_stats(y)
    z, _ = R.bn_act_fwd(y, mean, rstd, gamma, beta, act, keep, p)
    bw = R.bn_act_bwd(y, dz, mean, rstd, gamma, beta, act, keep, p)

    yt = torch.from_numpy(y).requires_grad_()
    gt, bt = torch.from_numpy(gamma).requires_grad_(), torch.from_numpy(beta).requires_grad_()
    pre = F.batch_norm(yt, None, None, gt, bt, True, 0.1, R.EPS)
    a = torch.relu(pre) if act == 1 else torch.tanh(pre)
    a = a * torch.from_numpy(keep.astype(np.float64)) * R.keep_scale(p)
    a.backward(torch.from_numpy(dz))
    errs = dict(z=_rel(z, a.detach().numpy()), dy=_rel(bw["dy"], yt.grad.numpy()), dgamma=_rel(bw["dgamma"], gt.grad.numpy()),
                dbeta=_rel(bw["dbeta"], bt.grad.numpy()))
    print(f"\n[reference] BatchNorm act {act} p {p} vs float64 autograd: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()) + " (tol 1e-12)")
    assert max(errs.values()) < 1e-12
    if p > 0:
        assert 0.5 < keep.mean() < 0.9 and not keep.all()


def test_bn_bwd_reference_two_parts_equal_whole_batch():
    """The data-parallel form: each part's dy from the summed sums and the global count equals the whole batch's dy."""
    rs = np.random.RandomState(5)
    c = 8
    y, dz = rs.standard_normal((30, c)) + 2, rs.standard_normal((30, c))
    gamma, beta = 1 + 0.1 * rs.standard_normal(c), 0.1 * rs.standard_normal(c)
    mean, var, rstd = R.bn_stats(y)
    whole = R.bn_act_bwd(y, dz, mean, rstd, gamma, beta, 2)
    parts = [R.bn_act_bwd(y[s], dz[s], mean, rstd, gamma, beta, 2) for s in (slice(0, 20), slice(20, 30))]
    sg, sgy = parts[0]["dbeta"] + parts[1]["dbeta"], parts[0]["dgamma"] + parts[1]["dgamma"]
    dy = np.concatenate([R.bn_act_bwd(y[s], dz[s], mean, rstd, gamma, beta, 2, sum_g=sg, sum_gy=sgy, count=30)["dy"]
                         for s in (slice(0, 20), slice(20, 30))])
    assert _rel(dy, whole["dy"]) < 1e-13 and _rel(sg, whole["dbeta"]) < 1e-13 and _rel(sgy, whole["dgamma"]) < 1e-13


@pytest.mark.parametrize("m", [2, 15, 262])
def test_running_statistics_reference_vs_batch_norm(m):
    rs = np.random.RandomState(m)
    c = 6
    y = rs.standard_normal((m, c)) * 3 - 4
    shift = rs.standard_normal(c)
    rm0, rv0 = rs.standard_normal(c), 1 + rs.rand(c)
    mean, var, rstd = R.bn_stats(y)
    rm, rv = R.bn_running(rm0, rv0, mean, var, m, shift)
    trm, trv = torch.from_numpy(rm0.copy()), torch.from_numpy(rv0.copy())
    out = F.batch_norm(torch.from_numpy(y + shift), trm, trv, None, None, True, 0.1, R.EPS)
    errs = (_rel(rm, trm.numpy()), _rel(rv, trv.numpy()), _rel((y - mean) * rstd, out.numpy()))
    print(f"\n[reference] running statistics, {m} rows vs F.batch_norm float64: mean {errs[0]:.1e} var {errs[1]:.1e} yhat {errs[2]:.1e} (tol 1e-12)")
    assert max(errs) < 1e-12
    rm_, rv_ = R.bn_running(rm0, rv0, mean, var, m)
    assert _rel(rm_, 0.9 * rm0 + 0.1 * mean) < 1e-15 and np.array_equal(rv_, rv)


def test_keep_mask_counters_and_seed_wrap():
    """The counters of the three index schemes and the 32-bit wrap of seed + seed_dev[0]."""
    idx = R.bn_idx(2, 3, 2, 4)
    assert idx.shape == (6, 4) and idx[0, 0] == 2 * 4 and idx[3, 1] == (7 + 2) * 4 + 1        # sample 1 starts at halo row 7
    assert np.array_equal(R.bn_idx(2, 3, 0, 4).reshape(-1), np.arange(24))
    assert np.array_equal(R.pe_idx(3, 4), np.arange(12).reshape(3, 4))
    i = np.arange(4096, dtype=np.uint64)
    a = R.keep_mask(0xFFFFFFF0, 0x20, 0.3, i)
    assert np.array_equal(a, R.keep_mask(0x10, None, 0.3, i)) and np.array_equal(a, R.keep_mask(0x10, 0, 0.3, i))
    assert np.array_equal(a, drop_hash(0x10, i) >= np.uint64(int(float(np.float32(0.3)) * 2 ** 32)))
    assert abs(a.mean() - 0.7) < 0.03 and R.keep_mask(1, 2, 0.0, i).all()
    assert not np.array_equal(a, R.keep_mask(0x11, None, 0.3, i))


@pytest.mark.parametrize("step,wd", [(1, 1e-2), (1000, 1e-2), (7, 0.0)])
def test_adamw_reference_vs_oracle(step, wd):
    g_ = torch.Generator().manual_seed(step)
    n = 257
    p, g = torch.randn(n, generator=g_, dtype=torch.float64), torch.randn(n, generator=g_, dtype=torch.float64) * 3
    m, v = torch.randn(n, generator=g_, dtype=torch.float64) * 0.1, torch.rand(n, generator=g_, dtype=torch.float64) * 0.1
    decay = (torch.rand(n, generator=g_) > 0.3).numpy().astype(np.uint8) * 255
    lr, b1, b2, eps, gscale = 3e-4, 0.9, 0.999, 1e-6, 0.25
    step_size = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
    got = R.adamw(p.numpy(), g.numpy(), m.numpy(), v.numpy(), decay, gscale, lr, step_size, b1, b2, eps, wd)
    p_ref, m_ref, v_ref = p.clone(), m.clone(), v.clone()
    for sel, w in ((torch.from_numpy(decay != 0), wd), (torch.from_numpy(decay == 0), 0.0)):
        ps, ms, vs = p_ref[sel], m_ref[sel], v_ref[sel]
        optim_ref.adamw_step(ps, g[sel] * gscale, ms, vs, step, lr, w, b1, b2, eps)
        p_ref[sel], m_ref[sel], v_ref[sel] = ps, ms, vs
    errs = (_rel(got["p"], p_ref.numpy()), _rel(got["m"], m_ref.numpy()), _rel(got["v"], v_ref.numpy()))
    print(f"\n[reference] AdamW step {step} wd {wd} vs oracle/optim_ref float64: p {errs[0]:.1e} m {errs[1]:.1e} v {errs[2]:.1e} (tol 1e-13)")
    assert max(errs) < 1e-13


@pytest.mark.parametrize("max_norm", [0.0, 1.0, 1e3])
def test_clip_reference_vs_oracle(max_norm):
    g = torch.randn(1000, generator=torch.Generator().manual_seed(0), dtype=torch.float64) * 3
    mult = 0.25
    norm = R.grad_norm(g.numpy(), mult)
    assert abs(norm - float((g * mult).norm())) < 1e-12 * norm
    want = mult * optim_ref.clip_coef([g * mult], max_norm)
    assert abs(R.clip_scale(norm, mult, max_norm) - want) < 1e-15
