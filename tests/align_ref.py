"""``rtts_align_stats`` and ``rtts_align_mas`` (include/rtts.h) restated in float64 numpy from their definitions -- TEST HELPER, not
the product: loops over the frames with ``np.log`` and ``np.exp``, nothing shared with csrc/align.hip.  Also the generators of the
test matrices."""
import itertools

import numpy as np

NAN = float("nan")


def scorable(a, t, k, mas=False):
    """The slot's region exists and is finite (and, for the search, holds a monotonic path over every key)."""
    tq, tk = a.shape
    if not (1 <= t <= tq and 1 <= k <= tk):
        return False
    if mas and t < k:
        return False
    return bool(np.isfinite(a[:t, :k]).all())


def stats_ref(a, t, k, sigma):
    """One slot of rtts_align_stats: ``a`` f32 (Tq, Tk), T = t, K = k -> (argmax (Tq,), dur_argmax (Tk,), row (8,) f64)."""
    tq, tk = a.shape
    argmax = np.full(tq, -1, dtype=np.int32)
    dur = np.zeros(tk, dtype=np.int32)
    if not scorable(a, t, k):
        return argmax, dur, np.full(8, NAN)
    total = peak = entropy = guided = 0.0
    cols = np.arange(k, dtype=np.float64)
    for i in range(t):
        row = a[i, :k].astype(np.float64)
        argmax[i] = int(np.argmax(a[i, :k]))                   # numpy: the first of equal maxima
        total += float(row.sum())
        peak += float(row.max())
        pos = row[row > 0]
        entropy += float(-(pos * np.log(pos)).sum())
        w = 1.0 - np.exp(-((cols / k - i / t) ** 2) / (2.0 * sigma * sigma))
        guided += float((row * w).sum())
    for i in range(t):
        dur[argmax[i]] += 1
    mono = sum(1 for i in range(1, t) if argmax[i] >= argmax[i - 1])
    cover = int((dur > 0).sum())
    return argmax, dur, np.array([t, k, total, peak, entropy, guided, mono, cover], dtype=np.float64)


def stats_batch_ref(mats, n_frames, n_keys, sigma):
    """``mats`` (L, B, Tq, Tk) f32 -> argmax (L, B, Tq), dur (L, B, Tk), table (L, B + 1, 8) with the totals row."""
    nl, nb, tq, tk = mats.shape
    argmax = np.empty((nl, nb, tq), dtype=np.int32)
    dur = np.empty((nl, nb, tk), dtype=np.int32)
    table = np.empty((nl, nb + 1, 8))
    for m in range(nl):
        for b in range(nb):
            argmax[m, b], dur[m, b], table[m, b] = stats_ref(mats[m, b], int(n_frames[b]), int(n_keys[b]), sigma)
        acc = np.zeros(8)
        for b in range(nb):
            acc = acc + table[m, b]
        table[m, nb] = acc
    return argmax, dur, table


def mas_ref(a, t, k, floor=1e-30):
    """One slot of rtts_align_mas -> (durations (Tk,), path (Tq,), [Q[T-1, K-1], sum_t a[t, k(t)]], decision margin): the margin
    is the smallest |Q[t-1, k] - Q[t-1, k-1]| met on the back-tracked path (inf when no decision was open)."""
    tq, tk = a.shape
    dur = np.zeros(tk, dtype=np.int32)
    path = np.full(tq, -1, dtype=np.int32)
    if not scorable(a, t, k, mas=True):
        return dur, path, np.array([NAN, NAN]), NAN
    c = np.log(np.maximum(a[:t, :k].astype(np.float64), floor))
    q = np.full((t, k), -np.inf)
    q[0, 0] = c[0, 0]
    move = np.full(k, -np.inf)
    for i in range(1, t):
        move[1:] = q[i - 1, :-1]                               # Q[t-1, k-1]; none for k = 0
        q[i] = c[i] + np.maximum(q[i - 1], move)               # -inf + c stays -inf right of the diagonal
    margin = np.inf
    j = k - 1
    for i in range(t - 1, -1, -1):
        path[i] = j
        if i == 0:
            break
        stay = q[i - 1, j]
        move = q[i - 1, j - 1] if j > 0 else -np.inf
        if np.isfinite(stay) and np.isfinite(move):
            margin = min(margin, abs(stay - move))
        if move > stay:                                        # a tie stays
            j -= 1
    assert j == 0
    for i in range(t):
        dur[path[i]] += 1
    mass = 0.0
    for i in range(t):
        mass += float(a[i, path[i]])
    return dur, path, np.array([q[t - 1, k - 1], mass]), margin


def mas_batch_ref(mats, n_frames, n_keys, floor=1e-30):
    """-> durations (L, B, Tk), path (L, B, Tq), scores (L, B + 1, 2), margins (L, B)."""
    nl, nb, tq, tk = mats.shape
    dur = np.empty((nl, nb, tk), dtype=np.int32)
    path = np.empty((nl, nb, tq), dtype=np.int32)
    scores = np.empty((nl, nb + 1, 2))
    margins = np.empty((nl, nb))
    for m in range(nl):
        for b in range(nb):
            dur[m, b], path[m, b], scores[m, b], margins[m, b] = mas_ref(mats[m, b], int(n_frames[b]), int(n_keys[b]), floor)
        acc = np.zeros(2)
        for b in range(nb):
            acc = acc + scores[m, b]
        scores[m, nb] = acc
    return dur, path, scores, margins


def mas_brute_force(a, t, k, floor=1e-30):
    """Every monotonic surjective path k(0) = 0, k(T-1) = K-1, steps 0 or 1 -> (best score, the set of best paths)."""
    c = np.log(np.maximum(a[:t, :k].astype(np.float64), floor))
    best, paths = -np.inf, []
    for ups in itertools.combinations(range(1, t), k - 1):      # the frames at which the path moves on
        path = np.zeros(t, dtype=np.int64)
        for u in ups:
            path[u:] += 1
        score = 0.0
        for i in range(t):
            score += c[i, path[i]]
        if score > best + 1e-12:
            best, paths = score, [tuple(path)]
        elif abs(score - best) <= 1e-12:
            paths.append(tuple(path))
    return best, paths


# ------------------------------------------------------------------ generators (f32 (Tq, Tk))
def noisy_diagonal(tq, tk, t, k, sharp, noise, seed):
    """softmax over k < K of -sharp (k / K - t / T)^2 + noise * N(0, 1), zero outside the region."""
    rng = np.random.default_rng(seed)
    a = np.zeros((tq, tk), dtype=np.float32)
    if t < 1 or k < 1:
        return a
    tt = np.arange(t)[:, None] / t
    kk = np.arange(k)[None, :] / k
    logits = -sharp * (kk - tt) ** 2 + noise * rng.standard_normal((t, k))
    logits -= logits.max(axis=1, keepdims=True)
    p = np.exp(logits)
    a[:t, :k] = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    return a


def pure_noise(tq, tk, seed):
    """Rows of uniform noise normalised to sum 1 over all Tk columns (a slot then sees the first K of them)."""
    rng = np.random.default_rng(seed)
    p = rng.random((tq, tk)) + 1e-3
    return (p / p.sum(axis=1, keepdims=True)).astype(np.float32)


def dyadic(tq, tk, t, k, seed, ridge=True):
    """Entries are multiples of 2^-10 and each of the first t rows sums to 1 over its first k columns (zero elsewhere): 1024 units
    dealt to random columns (with ``ridge``, half of them to a column that drifts along the region's diagonal).  Every f64 sum of
    such values is exact in any order."""
    rng = np.random.default_rng(seed)
    a = np.zeros((tq, tk), dtype=np.float32)
    for i in range(t):
        units = np.zeros(k, dtype=np.int64)
        free = 1024
        if ridge:
            units[min(k - 1, (i * k) // t)] += 512
            free = 512
        np.add.at(units, rng.integers(0, k, size=free), 1)
        a[i, :k] = (units / 1024.0).astype(np.float32)
    return a


def constant(tq, tk, value=2.0 ** -7):
    return np.full((tq, tk), value, dtype=np.float32)
