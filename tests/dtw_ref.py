"""``rtts_dtw_align`` (include/rtts.h) restated in float64 numpy from its definition -- TEST HELPER, not the product, and not a
port of anything: the projection, the frame distance from the differences, the recurrence with its tie-break order, the path
length.  Two more numbers come out of it that say how far another summation order may move the result:

  margin   the smallest gap, along the optimal path, between the chosen predecessor and the runner-up (inf where a cell has
           only one predecessor): a perturbation of the table below margin / 2 cannot change the path, so ``steps`` is only
           comparable where the margin is clear of the rounding noise
  E        the largest absolute difference between the table D built from the float64 distances and the same table built from
           those distances rounded to float32: the size of that noise

The table is walked by anti-diagonals (every cell of one depends only on the two before), vectorised over the diagonal."""
import numpy as np


def project(x, basis):
    """x (n_mel, T) f32, basis (n_proj, n_mel) f32 or None -> (T, n_proj) f32: p[k] = f32(sum_m f64(basis[k, m]) f64(x[m])), the sum
    taken with m ascending."""
    x = np.asarray(x, dtype=np.float32)
    if basis is None:
        return np.ascontiguousarray(x.T)
    basis = np.asarray(basis, dtype=np.float32)
    acc = np.zeros((x.shape[1], basis.shape[0]), dtype=np.float64)
    for m in range(x.shape[0]):
        acc += x[m].astype(np.float64)[:, None] * basis[:, m].astype(np.float64)[None, :]
    return acc.astype(np.float32)


def distances(p, q):
    """p (N, K), q (M, K) f32 -> (N, M) f64: sqrt(sum_k (p_i[k] - q_j[k])^2) from the differences, in float64."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    acc = np.zeros((p.shape[0], q.shape[0]), dtype=np.float64)
    for k in range(p.shape[1]):
        diff = p[:, k][:, None] - q[:, k][None, :]
        acc += diff * diff
    return np.sqrt(acc)


def table(d):
    """d (N, M) f64 -> D, S, choice (0 diagonal, 1 above, 2 left, -1 the origin), gap (runner-up minus chosen predecessor)."""
    n, m = d.shape
    big = np.inf
    dp = np.full((n + 1, m + 1), big)                        # D with a border of "no such cell" in front of row 0 and column 0
    sp = np.zeros((n + 1, m + 1), dtype=np.int64)
    choice = np.full((n, m), -1, dtype=np.int8)
    gap = np.full((n, m), big)
    dp[1, 1] = d[0, 0]
    sp[1, 1] = 1
    for k in range(1, n + m - 1):
        i = np.arange(max(0, k - m + 1), min(n - 1, k) + 1)
        j = k - i
        cand = np.stack([dp[i, j], dp[i, j + 1], dp[i + 1, j]])                  # diagonal, above, left
        steps = np.stack([sp[i, j], sp[i, j + 1], sp[i + 1, j]])
        best, c = cand[0].copy(), np.zeros(len(i), dtype=np.int8)
        for o in (1, 2):                                                         # a later one replaces only when strictly smaller
            take = cand[o] < best
            best[take], c[take] = cand[o][take], o
        ordered = np.sort(cand, axis=0)
        with np.errstate(invalid="ignore"):
            g = ordered[1] - ordered[0]
        gap[i, j] = np.where(np.isfinite(ordered[1]), g, big)
        choice[i, j] = c
        dp[i + 1, j + 1] = best + d[i, j]
        sp[i + 1, j + 1] = steps[c, np.arange(len(i))] + 1
    return dp[1:, 1:], sp[1:, 1:], choice, gap


def path(choice):
    """The optimal path, from the last cell back to the origin, as a list of (i, j)."""
    i, j = choice.shape[0] - 1, choice.shape[1] - 1
    cells = [(i, j)]
    while (i, j) != (0, 0):
        c = choice[i, j]
        i, j = (i - 1, j - 1) if c == 0 else (i - 1, j) if c == 1 else (i, j - 1)
        cells.append((i, j))
    return cells


def dtw(p, q):
    """Projected frames p (N, K), q (M, K) f32 -> dict(cost, steps, margin, E)."""
    d = distances(p, q)
    big_d, big_s, choice, gap = table(d)
    cells = path(choice)
    assert len(cells) == big_s[-1, -1]
    rounded, _, _, _ = table(d.astype(np.float32).astype(np.float64))
    return dict(cost=float(big_d[-1, -1]), steps=int(big_s[-1, -1]), margin=float(min(gap[c] for c in cells)),
                E=float(np.max(np.abs(big_d - rounded))))


def align(gens, truths, basis=None):
    """Lists of (n_mel, N_b) and (n_mel, M_b) f32 arrays -> (cost (B,), steps (B,), totals (2,), per-slot dicts)."""
    slots = [dtw(project(g, basis), project(t, basis)) for g, t in zip(gens, truths)]
    cost = np.array([s["cost"] for s in slots])
    steps = np.array([s["steps"] for s in slots], dtype=np.int64)
    return cost, steps, np.array([np.mean(cost / steps), cost.sum() / steps.sum()]), slots


def cepstral_basis(n_mel, n_coef=13):
    """evaluation.cepstral_basis, written out again: rows 1..n_coef of the orthonormal DCT-II times (10 / ln 10) sqrt 2, float64."""
    k = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mel, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / n_mel) * np.cos(np.pi * k * (m + 0.5) / n_mel) * (10.0 / np.log(10.0) * np.sqrt(2.0))


def brute_force(d):
    """Every monotone path from (0, 0) to the last cell of d (N, M), N, M <= 5: -> (minimum cost, steps of THE path the
    tie-break order picks).  Read from the end, the recurrence prefers the diagonal to the cell above to the cell on the left
    among the predecessors an optimal path runs through: of all minimum-cost paths, the one whose moves, last first, are
    smallest in that order."""
    n, m = d.shape
    found = []

    def walk(i, j, cost, moves):
        cost = cost + d[i, j]
        if (i, j) == (n - 1, m - 1):
            found.append((cost, tuple(reversed(moves))))
            return
        if i + 1 < n and j + 1 < m:
            walk(i + 1, j + 1, cost, moves + [0])
        if i + 1 < n:
            walk(i + 1, j, cost, moves + [1])
        if j + 1 < m:
            walk(i, j + 1, cost, moves + [2])
    walk(0, 0, 0.0, [])
    low = min(c for c, _ in found)
    return low, len(min(mv for c, mv in found if c == low)) + 1


def warped_case(rng, n_mel=80):
    """A truth of M in 33..160 frames -- a random walk over time plus per-channel noise around -5, like a log-mel -- and a
    generation of N frames, |N - M| <= 25: the truth resampled (linear interpolation) at N sorted random positions, plus noise
    of 0.3 of the truth's standard deviation.  -> (gen (n_mel, N), truth (n_mel, M)) f32."""
    m = int(rng.integers(33, 161))
    n = int(np.clip(m + rng.integers(-25, 26), 8, None))
    walk = np.cumsum(rng.standard_normal((n_mel, m)) * 0.4, axis=1)
    truth = (-5.0 + walk + rng.standard_normal((n_mel, m)) * 0.5).astype(np.float32)
    pos = np.sort(rng.uniform(0, m - 1, size=n))
    lo = np.floor(pos).astype(np.int64)
    hi = np.minimum(lo + 1, m - 1)
    frac = (pos - lo)[None, :]
    gen = truth[:, lo] * (1 - frac) + truth[:, hi] * frac + rng.standard_normal((n_mel, n)) * 0.3 * float(truth.std())
    return gen.astype(np.float32), truth
