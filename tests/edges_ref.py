"""Plain float64 references of the kernels of csrc/edges.hip around the convolutions and of csrc/optim.hip (TEST INFRASTRUCTURE).

numpy on the CPU only; no project kernel is called.  Arrays are float64 unless stated; "plain rows" are (B*L, C).
tests/test_edges_ref_cpu.py checks these functions against torch.autograd, F.batch_norm and oracle/optim_ref.py in float64."""
import numpy as np

from oracle.synth import drop_hash

EPS = 1e-5                 # BatchNorm eps of the kernels
MOMENTUM = 0.1
U24 = 2.0 ** -24           # float32 unit roundoff
U9 = 2.0 ** -9             # relu_drop: scaling by a power of two is exact, any rounding at all would exceed this
BF16_U = 2.0 ** -8         # bf16 unit roundoff: 8 significant bits, half an ulp is up to 2^-8 of the value (just above a power of two)


# ------------------------------------------------------------------ dropout masks
def keep_mask(seed: int, seed_dev, p: float, idx):
    """bool array like idx: element kept iff drop_hash(seed_eff, idx) >= uint32(float32(p) * 2^32); seed_eff = (seed + seed_dev[0])
    mod 2^32 (seed_dev None: seed alone).  p = 0 keeps everything."""
    idx = np.asarray(idx, dtype=np.uint64)
    if p <= 0:
        return np.ones(idx.shape, dtype=bool)
    seed_eff = (int(seed) + (0 if seed_dev is None else int(seed_dev))) % (1 << 32)
    thresh = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    return drop_hash(seed_eff, idx) >= thresh


def keep_scale(p: float) -> float:
    return 1.0 / (1.0 - float(np.float32(p)))


def bn_idx(b: int, l: int, halo: int, c: int):
    """(B*L, C) dropout counters of the BatchNorm kernels: (row of y in halo rows, no lead-in) * C + channel."""
    rows = (np.arange(b)[:, None] * (l + 2 * halo) + halo + np.arange(l)[None, :]).reshape(-1)
    return rows[:, None].astype(np.uint64) * np.uint64(c) + np.arange(c, dtype=np.uint64)[None, :]


def pe_idx(t: int, d: int):
    """(T, d) dropout counters of rtts_pe_add / rtts_pe_dalpha: t * d + c, shared over the batch."""
    return np.arange(t * d, dtype=np.uint64).reshape(t, d)


# ------------------------------------------------------------------ BatchNorm
def bn_stats(y):
    """y (M, C) -> mean, biased variance, rstd = (var + eps)^-1/2 over the rows, two-pass in float64."""
    y = np.asarray(y, dtype=np.float64)
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    return mean, var, 1.0 / np.sqrt(var + EPS)


def bn_running(run_mean, run_var, mean, var, m: int, mean_shift=None):
    """Running statistics after one batch: momentum 0.1, unbiased variance; mean_shift (the conv bias kept out of y) moves the
    running mean only."""
    shift = 0.0 if mean_shift is None else np.asarray(mean_shift, dtype=np.float64)
    rm = (1 - MOMENTUM) * np.asarray(run_mean, dtype=np.float64) + MOMENTUM * (mean + shift)
    rv = (1 - MOMENTUM) * np.asarray(run_var, dtype=np.float64) + MOMENTUM * var * (m / max(m - 1, 1))
    return rm, rv


def _act(pre, act: int):
    return np.maximum(pre, 0.0) if act == 1 else np.tanh(pre)


def _dact(pre, act: int):
    return (pre > 0).astype(np.float64) if act == 1 else 1.0 - np.tanh(pre) ** 2


def bn_act_fwd(y, mean, rstd, gamma, beta, act: int, keep=None, p: float = 0.0):
    """z = keep * act(gamma * (y - mean) * rstd + beta) / (1 - p) on plain rows -> (z, pre)."""
    y = np.asarray(y, dtype=np.float64)
    pre = gamma * ((y - mean) * rstd) + beta
    z = _act(pre, act)
    if keep is not None:
        z = z * keep * keep_scale(p)
    return z, pre


def bn_act_bwd(y, dz, mean, rstd, gamma, beta, act: int, keep=None, p: float = 0.0, sum_g=None, sum_gy=None, count=None):
    """BatchNorm(train) backward through act and dropout on plain rows:
        g = dz * act' * keep/(1-p);  dbeta = sum g;  dgamma = sum g*yhat;  dy = gamma*rstd*(g - sum g/M - yhat * sum(g*yhat)/M).
    sum_g / sum_gy / count given: the sums of the WHOLE batch (data parallel), y then being one rank's part.
    -> dict(dy, dgamma, dbeta, g, yhat, pre); dgamma / dbeta are those of THIS y."""
    y = np.asarray(y, dtype=np.float64)
    yhat = (y - mean) * rstd
    pre = gamma * yhat + beta
    g = np.asarray(dz, dtype=np.float64) * _dact(pre, act)
    if keep is not None:
        g = g * keep * keep_scale(p)
    dbeta, dgamma = g.sum(0), (g * yhat).sum(0)
    sg = dbeta if sum_g is None else sum_g
    sgy = dgamma if sum_gy is None else sum_gy
    m = y.shape[0] if count is None else count
    dy = gamma * rstd * (g - sg / m - yhat * sgy / m)
    return dict(dy=dy, dgamma=dgamma, dbeta=dbeta, g=g, yhat=yhat, pre=pre)


# ------------------------------------------------------------------ positional encoding, relu + dropout
def pe_add(y, table, alpha: float, keep=None, p: float = 0.0):
    """y (B, T, d) + alpha * keep/(1-p) * table (T, d)."""
    t = np.asarray(table, dtype=np.float64)
    if keep is not None:
        t = t * keep * keep_scale(p)
    return np.asarray(y, dtype=np.float64) + alpha * t[None]


def pe_dalpha(dy, table, keep=None, p: float = 0.0):
    """-> (sum dy * table * keep/(1-p), sum |dy * table * keep/(1-p)|) over (B, T, d)."""
    t = np.asarray(table, dtype=np.float64)
    if keep is not None:
        t = t * keep * keep_scale(p)
    prod = np.asarray(dy, dtype=np.float64) * t[None]
    return prod.sum(), np.abs(prod).sum()


def relu_drop(h, keep=None, p: float = 0.0):
    out = np.maximum(np.asarray(h, dtype=np.float64), 0.0)
    if keep is not None:
        out = out * keep * keep_scale(p)
    return out


# ------------------------------------------------------------------ optimizer (the header of csrc/optim.hip)
def grad_norm(g, grad_mult: float = 1.0) -> float:
    g = np.asarray(g, dtype=np.float64)
    return float(np.sqrt((g * g).sum())) * grad_mult


def clip_scale(norm: float, grad_mult: float, max_norm: float) -> float:
    """scale[0] of rtts_grad_clip_scale from the (already multiplied) norm: grad_mult * min(1, max_norm / (norm + 1e-6));
    max_norm <= 0: no clip."""
    return grad_mult * (1.0 if max_norm <= 0 else min(1.0, max_norm / (norm + 1e-6)))


def adamw(p, g, m, v, decay, gscale: float, lr: float, step_size: float, b1: float, b2: float, eps: float, wd: float):
    """m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= step_size m / (sqrt(v) + eps); then p -= lr wd p where decay != 0
    (decoupled, on the updated p); g is the stored gradient times gscale.  -> p, m, v and the two terms of each sum."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g = g * gscale
    m1a, m1b = b1 * m, (1 - b1) * g
    v1a, v1b = b2 * v, (1 - b2) * g * g
    m1, v1 = m1a + m1b, v1a + v1b
    upd = step_size * m1 / (np.sqrt(v1) + eps)
    p1 = p - upd
    p1 = np.where(np.asarray(decay) != 0, p1 - lr * wd * p1, p1)
    return dict(p=p1, m=m1, v=v1, m_terms=np.abs(m1a) + np.abs(m1b), v_terms=np.abs(v1a) + np.abs(v1b), v_g=np.abs(v1b), upd=upd)
