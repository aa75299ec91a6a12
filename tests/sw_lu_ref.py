"""float64 restatement of ``rtts_sw_inv1x1_factor`` (csrc/sw_lu.hip) -- TEST HELPER, not the product -- with the matrices and
the bounds its tests use.

``factor`` is the kernel's algorithm in numpy: W widened to float64, Gauss-Jordan elimination in place with partial (row)
pivoting -- the largest |a| of the column, the LOWEST row on a tie --, log|det| the sum of log|pivot| in pivot order, the sign the
permutation's parity times the pivots' signs, the row permutation undone on the way out, W^-1 rounded to fp32 once.  A pivot that
is exactly 0: sign 0, -inf, an all-NaN inverse.  (The kernel contracts a - f * r into one fused multiply-add; numpy rounds twice:
the two agree within the bounds, not bit for bit.)

The reference of every test is LAPACK on the fp32 weights widened to float64 (``np.linalg.slogdet`` / ``np.linalg.inv``), with
kappa = ``np.linalg.cond(W)`` and u64 = 2^-53:

    log-det      |got - ref| <= 8 n^2 u64 kappa        d log det = tr(W^-1 dW) with a backward-stable elimination
                                                       (|dW| <~ n u64 |W|: n^2 terms of at most kappa u64 each), margin 8
    inverse      |got32 - inv64| <= 2^-24 |inv64| + 8 n u64 kappa ||inv64||_2      element-wise: the one rounding to fp32, and the
                                                       float64 error of a backward-stable inverse, margin 8
    sign         exact"""
from __future__ import annotations

from typing import Tuple

import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24
SIZES = (1, 2, 6, 8, 48, 112, 128)
KINDS = ("orthonormal", "gaussian", "kappa1e5", "pivoting")
CASES = tuple((k, n) for k in KINDS for n in SIZES if not (k == "pivoting" and n % 2))     # a 1 x 1 matrix has no rows to exchange
DEFAULT_MODEL_SIZES = (128, 128, 112, 112, 96, 96, 80, 80, 64, 64, 48, 48)     # the twelve flows of the default SqueezeWave


def factor(w32: np.ndarray) -> Tuple[np.ndarray, float, float]:
    """-> (W^-1 fp32, sign in {-1, 0, +1}, log|det W|) by the kernel's algorithm."""
    a = np.array(w32, dtype=np.float64)
    n = a.shape[0]
    assert a.shape == (n, n) and n >= 1
    perm = np.arange(n)
    sign, logabs = 1.0, 0.0
    for k in range(n):
        col = np.abs(a[k:, k])
        p = k + int(np.argmax(col))                       # argmax returns the FIRST maximum: the lowest row on a tie
        pivot = a[p, k]
        if pivot == 0.0:
            return np.full((n, n), np.nan, dtype=np.float32), 0.0, -np.inf
        logabs += np.log(abs(pivot))
        if pivot < 0:
            sign = -sign
        if p != k:
            sign = -sign
            a[[k, p]] = a[[p, k]]
            perm[[k, p]] = perm[[p, k]]
        row = a[k] / pivot
        row[k] = 1.0 / pivot
        f = a[:, k].copy()
        a[:, k] = 0.0
        a -= np.outer(f, row)
        a[k] = row
    inv = np.empty_like(a)
    inv[:, perm] = a                                      # R = W^-1 P^T: column r of R is column perm[r] of W^-1
    return inv.astype(np.float32), sign, logabs


def _orth(n: int, rng: np.random.Generator) -> np.ndarray:
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def matrix(kind: str, n: int, seed: int = 0) -> np.ndarray:
    """The fp32 test matrices.  ``orthonormal``: Q * 1.3 + 0.01 (what an InvertibleConv1d looks like early in training);
    ``gaussian``; ``kappa1e5``: U diag(logspace(0, -5, n)) V^T with U, V the orthonormal factors of seeded Gaussian matrices;
    ``pivoting`` (n even): a diagonally dominant matrix with its rows shifted by one (an n-cycle: an ODD permutation for even
    n) and every entry of the leading diagonal set to zero -- every step must change rows, and the determinant is negative."""
    rng = np.random.default_rng(1000 * n + 17 * seed + KINDS.index(kind) if kind in KINDS else seed)
    if kind == "orthonormal":
        w = _orth(n, rng) * 1.3 + 0.01
    elif kind == "gaussian":
        w = rng.standard_normal((n, n))
    elif kind == "kappa1e5":
        w = _orth(n, rng) @ np.diag(np.logspace(0, -5, n)) @ _orth(n, rng).T
    elif kind == "pivoting":
        assert n % 2 == 0, "an n-cycle is odd for even n only"
        b = np.diag(1.0 + rng.random(n)) + 0.1 / n * rng.standard_normal((n, n))
        w = np.roll(b, 1, axis=0)                         # row i of w = row i - 1 of b: no row keeps its place
        w[np.arange(n), np.arange(n)] = 0.0
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(w.astype(np.float32))


def singular(n: int, seed: int = 0) -> np.ndarray:
    """A Gaussian matrix with one column set to zero: elimination meets a column of exact zeros."""
    w = matrix("gaussian", n, seed + 5)
    w[:, n // 3] = 0.0
    return w


def reference(w32: np.ndarray):
    """-> (sign, log|det|, inv64, kappa, log-det tolerance, element-wise inverse tolerance) from LAPACK in float64."""
    w = w32.astype(np.float64)
    n = w.shape[0]
    sign, logabs = np.linalg.slogdet(w)
    inv = np.linalg.inv(w)
    kappa = float(np.linalg.cond(w))
    tol_ld = 8.0 * n * n * U64 * kappa
    tol_inv = U32 * np.abs(inv) + 8.0 * n * U64 * kappa * np.linalg.norm(inv, 2)
    return float(sign), float(logabs), inv, kappa, tol_ld, tol_inv


def ratios(inv32: np.ndarray, sign: float, logabs: float, w32: np.ndarray):
    """-> (sign matches the reference, log-det error / bound, worst inverse error / bound, the reference's sign)."""
    rsign, rlog, inv, _, tol_ld, tol_inv = reference(w32)
    r_ld = abs(logabs - rlog) / tol_ld
    r_inv = float(np.max(np.abs(inv32.astype(np.float64) - inv) / tol_inv))
    return sign == rsign, r_ld, r_inv, rsign
