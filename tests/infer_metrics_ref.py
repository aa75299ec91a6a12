"""float64 numpy restatement of ``rtts_infer_metrics`` (include/rtts.h): the inference_pred_mse / inference_stop_mae of the
reference's ``LitReformerTTS.validate_inference`` (``training/wrappers.py:188-195``) and the per-utterance squared error behind
``predict_samples``' ``mse_loss`` (``cli.py:150``).  A test helper, not a test."""
import numpy as np


def infer_metrics(gen, gen_stop, truths, lm):
    """gen: (B, n_mel, L) array of generated frames; gen_stop: (B,) ints or None; truths: B arrays (n_mel, len_b); lm: the
    batch's longest truth.  -> (sse (B,), stop_err (B,), totals (2,)) in float64:
        sse[b]      = sum_{t < len_b} sum_m ([t < L] gen[b, m, t] - truth_b[m, t])^2
        stop_err[b] = |gen_stop[b] - (len_b - 1)|                    (0 without gen_stop)
        totals      = [sum_b sse[b] / (B n_mel lm), mean_b stop_err[b]]"""
    gen = np.asarray(gen, dtype=np.float64)
    b, n_mel, frames = gen.shape
    sse, stop_err = np.zeros(b), np.zeros(b)
    for i, truth in enumerate(truths):
        truth = np.asarray(truth, dtype=np.float64)
        n = truth.shape[1]
        padded = np.zeros((n_mel, n))
        padded[:, :min(n, frames)] = gen[i, :, :min(n, frames)]
        sse[i] = ((padded - truth) ** 2).sum()
        if gen_stop is not None:
            stop_err[i] = abs(int(gen_stop[i]) - (n - 1))
    return sse, stop_err, np.array([sse.sum() / (b * n_mel * lm), stop_err.mean()])


def make_case(n_mel, lengths, frames, seed=0):
    """Log-mel-like truths of the given lengths, a generated (B, n_mel, frames) spectrogram and stop indices, all float32 /
    int64 numpy arrays."""
    rng = np.random.RandomState(seed + 1000 * n_mel + frames)
    truths = [np.clip(rng.standard_normal((n_mel, n)) * 2 - 5, -11.5, 2.0).astype(np.float32) for n in lengths]
    gen = np.clip(rng.standard_normal((len(lengths), n_mel, frames)) * 2 - 5, -11.5, 2.0).astype(np.float32)
    stop = rng.randint(1, max(frames, 2) + 1, size=len(lengths)).astype(np.int64)
    return gen, stop, truths


def collate(truths):
    """``custom_sequence_padder``'s spectrogram side for these truths: spectrogram (B, 1 + lm, n_mel) behind a zero start frame,
    stop_tokens (B, lm), loss_mask (B, lm, n_mel), float32."""
    b, n_mel, lm = len(truths), truths[0].shape[0], max(t.shape[1] for t in truths)
    spec = np.zeros((b, lm + 1, n_mel), np.float32)
    stop = np.zeros((b, lm), np.float32)
    mask = np.zeros((b, lm, n_mel), np.float32)
    for i, t in enumerate(truths):
        n = t.shape[1]
        spec[i, 1:n + 1] = t.T
        stop[i, n - 1] = 1.0
        mask[i, :n] = 1.0
    return spec, stop, mask
