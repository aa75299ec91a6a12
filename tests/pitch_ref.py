"""``rtts_pitch_yin`` and ``rtts_f0_compare`` (include/rtts.h) restated in float64 numpy from their definitions -- TEST HELPER, not
the product, and not a port of anything: the difference function in its direct form, the cumulative-mean normalisation, the
threshold pick with its descent, the three-point interpolation, and the five counts of the contour comparison.

``yin_pick`` takes ANY d' array, so a test can apply it to the kernel's own f32 d' (where every comparison is exact and the pick
must agree at every frame) as well as to the float64 one.  Next to its results it says which frames are FRAGILE: a frame where a
comparison the pick made was between two numbers within 4e-4 relative of each other (twice the bound the kernel's d' is held
to), so that another summation order may legitimately decide it the other way.

The test signals are built here too, seeded, at 22,050 Hz."""
import numpy as np

W = 1024                 # integration window
MAX_LAG = 512            # RTTS_PITCH_MAX_LAG
REACH = W + MAX_LAG      # samples a frame reads: [t hop - REACH / 2, t hop + REACH / 2)
SR = 22050
FRAGILE = 4e-4

_IDX = np.arange(MAX_LAG + 1)[:, None] + np.arange(W)[None, :]


def frames_of(n, hop):
    return n // hop + 1


def _padded(x, hop):
    x = np.asarray(x, dtype=np.float64)
    t = frames_of(len(x), hop)
    xp = np.zeros(REACH // 2 + (t - 1) * hop + REACH // 2 + len(x) % hop + hop, dtype=np.float64)
    xp[REACH // 2: REACH // 2 + len(x)] = x
    return xp, t


def yin_cmnd(x, hop):
    """x (N,) -> (d' (T, 513) f64, d (T, 513) f64), T = N // hop + 1; zero outside the utterance."""
    xp, t = _padded(x, hop)
    d = np.empty((t, MAX_LAG + 1), dtype=np.float64)
    for f in range(t):
        seg = xp[f * hop: f * hop + REACH]
        diff = seg[None, :W] - seg[_IDX]
        d[f] = (diff * diff).sum(axis=1)
    run = np.cumsum(d[:, 1:], axis=1)
    cmnd = np.ones_like(d)
    tau = np.arange(1, MAX_LAG + 1, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        cmnd[:, 1:] = np.where(run == 0.0, 1.0, d[:, 1:] * tau / run)
    return cmnd, d


def touched(x, hop):
    """(T,) bool: the frames whose REACH samples hold a non-finite value."""
    xp, t = _padded(x, hop)
    bad = ~np.isfinite(xp)
    return np.array([bad[f * hop: f * hop + REACH].any() for f in range(t)])


def _close(p, q):
    return abs(p - q) <= FRAGILE * max(abs(p), abs(q))


def yin_pick(cmnd, tau_min, tau_max, thr, sr):
    """cmnd (T, 513), any float type -> dict of (T,) arrays: tau (0 = unvoiced), voiced, f0 and aperiodicity in float64 from the
    values given, fragile."""
    c = np.asarray(cmnd).astype(np.float64)
    n = c.shape[0]
    out = dict(tau=np.zeros(n, dtype=np.int64), voiced=np.zeros(n, dtype=bool), f0=np.zeros(n), aperiodicity=np.zeros(n),
               fragile=np.zeros(n, dtype=bool))
    for f in range(n):
        row = c[f]
        fragile, tau = False, 0
        for k in range(tau_min, tau_max + 1):
            fragile |= _close(row[k], thr)
            if row[k] < thr:
                tau = k
                break
        if tau == 0:
            out["aperiodicity"][f] = row[tau_min: tau_max + 1].min()
            out["fragile"][f] = fragile
            continue
        while tau + 1 <= tau_max:
            fragile |= _close(row[tau + 1], row[tau])
            if not row[tau + 1] < row[tau]:
                break
            tau += 1
        a, b, cc = row[tau - 1], row[tau], row[tau + 1]
        fragile |= _close(a, b) or _close(cc, b)
        off = 0.5 * (a - cc) / (a - 2.0 * b + cc) if (a > b and cc >= b) else 0.0
        out["tau"][f], out["voiced"][f], out["f0"][f], out["aperiodicity"][f], out["fragile"][f] = tau, True, sr / (tau + off), b, fragile
    return out


def f0_compare_ref(fa, offs_a, fb, offs_b, gross):
    """-> (B + 1, 5) f64: per utterance [frames compared, voiced in both, sum of squared cents, gross errors, voicing differences]
    over the first min(T_a, T_b) frames, the last row the column sums; a NaN frame makes its row (and the last) NaN."""
    nseg = len(offs_a) - 1
    table = np.zeros((nseg + 1, 5), dtype=np.float64)
    for s in range(nseg):
        n = min(offs_a[s + 1] - offs_a[s], offs_b[s + 1] - offs_b[s])
        a = np.asarray(fa[offs_a[s]: offs_a[s] + n], dtype=np.float64)
        b = np.asarray(fb[offs_b[s]: offs_b[s] + n], dtype=np.float64)
        if np.isnan(a).any() or np.isnan(b).any():
            table[s] = np.nan
            continue
        both = (a > 0) & (b > 0)
        ratio = a[both] / b[both]
        cents = 1200.0 * np.log2(ratio)
        table[s] = [n, both.sum(), (cents * cents).sum(), (np.abs(ratio - 1.0) > gross).sum(), ((a > 0) != (b > 0)).sum()]
    table[nseg] = table[:nseg].sum(axis=0)
    return table


# ---- the test signals ------------------------------------------------------------------------------------------------------------

def tone(f0, n, rng, harmonics=5, level=0.5):
    """``harmonics`` partials of f0 with amplitudes 1 / h and seeded phases, scaled so that the amplitudes add up to ``level``."""
    t = np.arange(n, dtype=np.float64) / SR
    amps = 1.0 / np.arange(1, harmonics + 1)
    amps *= level / amps.sum()
    x = np.zeros(n)
    for h, a in enumerate(amps, start=1):
        x += a * np.sin(2.0 * np.pi * h * f0 * t + rng.uniform(0.0, 2.0 * np.pi))
    return x


def glide(f_from, f_to, n, rng):
    """A linear glide of the fundamental with its octave at half the amplitude."""
    f = np.linspace(f_from, f_to, n)
    phase = 2.0 * np.pi * np.cumsum(f) / SR
    return 0.3 * np.sin(phase + rng.uniform(0.0, 2.0 * np.pi)) + 0.15 * np.sin(2.0 * phase + rng.uniform(0.0, 2.0 * np.pi))


def noise(n, rng, level=0.3):
    return level * rng.uniform(-1.0, 1.0, n)


STEADY = {"tone110": 110.0, "tone50": 50.0, "tone400": 400.0}


def signals(seed=2002):
    """The twelve utterances as f32 arrays, by name, in batch order: 181 frames at hop 256."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, f0 in STEADY.items():
        out[name] = tone(f0, 6000, rng)
    out["glide"] = glide(90.0, 300.0, 6000, rng)
    out["noise"] = noise(6000, rng)
    out["pause_tone_pause"] = np.concatenate([np.zeros(2000), tone(200.0, 3000, rng), np.zeros(1500)])
    out["tone_noise"] = tone(150.0, 6000, rng) + noise(6000, rng, 0.1)
    out["one"] = np.array([0.25])
    for n in (255, 256, 300, 1279):
        out[f"short{n}"] = tone(180.0, n, rng)
    return {k: v.astype(np.float32) for k, v in out.items()}


def seam_tone(tile_frames, hop=256, seed=7):
    """A tone of (2 tile_frames + 1) hop samples: its frames cross two tile seams."""
    return tone(130.0, (2 * tile_frames + 1) * hop, np.random.default_rng(seed)).astype(np.float32)
