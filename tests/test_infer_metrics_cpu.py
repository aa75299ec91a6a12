"""The float64 restatement of ``rtts_infer_metrics`` (tests/infer_metrics_ref.py) against the literal lines of the reference --
``training/wrappers.py:188-195`` and ``cli.py:150`` -- run in fp32 on the CPU, and the host-side argument checks of
``ops.infer_metrics``.  No GPU.

Tolerance: a sum of n non-negative fp32 terms accumulated in any order is within n * 2^-24 (relative) of the exact sum of those
terms: the batch metric is held to n * 2^-24 with n = B * n_mel * lm, the element count of the reference's mse_loss, computed by
the test.  The per-utterance check has as few as 7 terms, where the roundings of a term itself (the subtraction, the square:
3 * 2^-24) and of the division show: it is held to (n + 4) * 2^-24.  A semantic mistake (the wrong denominator, a frame counted
or dropped) is an error of order 1."""
import numpy as np
import pytest
import torch
from torch.nn.functional import mse_loss

import infer_metrics_ref as ref

U = 2.0 ** -24


def _reference_lines(mel_out, stop_out, batch):
    """wrappers.py:170-172 and :188-195, verbatim up to ``self.`` and ``.cuda()``."""
    true_mel = batch['spectrogram'][:, 1:, :].transpose(1, 2)
    true_mask = batch["loss_mask"].transpose(1, 2)
    true_stop = batch["stop_tokens"].argmax(dim=1)

    padded_mel_out = torch.zeros_like(true_mel)
    common_mel_len = min(padded_mel_out.shape[-1], mel_out.shape[-1])
    padded_mel_out[:, :, :common_mel_len] = mel_out[:, :, :common_mel_len]
    padded_mel_out *= true_mask
    inference_pred_mse = mse_loss(padded_mel_out, true_mel).cpu().item()

    inference_stop_mae = torch.abs(stop_out - true_stop) \
        .to(dtype=torch.float).mean().cpu().item()
    return inference_pred_mse, inference_stop_mae


@pytest.mark.parametrize("frames", [0, 1, 5, 9, 90, 400])
@pytest.mark.parametrize("lengths", [[6, 1, 9], [50, 120, 300]], ids=str)
@pytest.mark.parametrize("n_mel", [7, 80])
def test_restatement_is_the_reference_lines(n_mel, lengths, frames):
    gen, stop, truths = ref.make_case(n_mel, lengths, frames)
    spec, stop_tokens, mask = ref.collate(truths)
    batch = dict(spectrogram=torch.from_numpy(spec), stop_tokens=torch.from_numpy(stop_tokens), loss_mask=torch.from_numpy(mask))
    lm = max(lengths)
    want_mse, want_mae = _reference_lines(torch.from_numpy(gen), torch.from_numpy(stop), batch)
    sse, stop_err, totals = ref.infer_metrics(gen, stop, truths, lm)
    n = len(lengths) * n_mel * lm
    print(f"\n[restatement] n_mel {n_mel} lengths {lengths} L {frames}: mse {totals[0]:.9g} vs fp32 {want_mse:.9g}, rel "
          f"{abs(totals[0] - want_mse) / totals[0]:.2e} (bound {n * U:.2e}); stop mae {totals[1]} vs {want_mae}")
    assert abs(totals[0] - want_mse) <= n * U * totals[0]
    assert abs(totals[1] - want_mae) <= 4 * U * max(totals[1], 1.0)          # small integers: exact up to the fp32 mean
    assert np.array_equal(stop_err, np.abs(stop - (np.array(lengths) - 1)))


@pytest.mark.parametrize("n_mel,length", [(7, 1), (7, 9), (80, 120)])
def test_per_utterance_mse_is_cli_line_150(n_mel, length):
    """cli.py:150: ``mse_loss(spectrogram_out, spectrogram_in[:, 1:, :])`` at B = 1 over the utterance's own frames =
    sse[b] / (len_b * n_mel) of a teacher-forced prediction (as many frames as the truth)."""
    gen, _, truths = ref.make_case(n_mel, [length, length + 3], length + 3, seed=5)
    sse, _, _ = ref.infer_metrics(gen, None, truths, length + 3)
    for b, truth in enumerate(truths):
        n = truth.shape[1]
        spectrogram_out = torch.from_numpy(gen[b:b + 1, :, :n]).transpose(1, 2)
        spectrogram_in = torch.cat([torch.zeros(1, 1, n_mel), torch.from_numpy(truth.T).unsqueeze(0)], dim=1)
        mse = float(mse_loss(spectrogram_out, spectrogram_in[:, 1:, :]))
        got = sse[b] / (n * n_mel)
        assert abs(got - mse) <= (n * n_mel + 4) * U * got


def test_ops_refuses_bad_arguments_on_the_host():
    from reformer_tts_amd import _lib, ops
    gen, stop, truth = torch.zeros(2, 7, 5), torch.zeros(2, dtype=torch.int64), torch.zeros(7, 20)
    fo, ids = torch.tensor([0, 8, 20]), torch.tensor([1, 0], dtype=torch.int32)
    starts, lengths = torch.tensor([0, 8]), torch.tensor([8, 12], dtype=torch.int32)
    with pytest.raises(ValueError, match="exactly one"):                      # neither description
        ops.infer_metrics(gen, stop, truth, 12)
    with pytest.raises(ValueError, match="exactly one"):                      # both
        ops.infer_metrics(gen, stop, truth, 12, frame_offsets=fo, ids=ids, starts=starts, lengths=lengths)
    with pytest.raises(ValueError, match="exactly one"):                      # half of the padded-batch description
        ops.infer_metrics(gen, stop, truth, 12, starts=starts)
    with pytest.raises(ValueError, match="exactly one"):                      # ids belong to the corpus description
        ops.infer_metrics(gen, stop, truth, 12, ids=ids, starts=starts, lengths=lengths)
    for bad in (dict(gen=gen.double()), dict(gen_stop=stop.int()), dict(truth=truth.half())):
        args = dict(gen=gen, gen_stop=stop, truth=truth)
        args.update(bad)
        with pytest.raises(ValueError, match="must be a torch"):
            ops.infer_metrics(args["gen"], args["gen_stop"], args["truth"], 12, frame_offsets=fo, ids=ids)
    with pytest.raises(ValueError, match="ids must be a torch.int32"):
        ops.infer_metrics(gen, stop, truth, 12, frame_offsets=fo, ids=ids.long())
    with pytest.raises(ValueError, match="lengths must be a torch.int32"):
        ops.infer_metrics(gen, stop, truth, 12, starts=starts, lengths=lengths.long())
    with pytest.raises(_lib.RttsError, match="GPU only"):                     # everything right but the device
        ops.infer_metrics(gen, stop, truth, 12, frame_offsets=fo, ids=ids)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        ops.infer_metrics(gen, None, truth, 12, starts=starts, lengths=lengths)
