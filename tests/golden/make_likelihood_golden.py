#!/usr/bin/env python3
"""Generate ``squeezewave_likelihood.npz`` FROM THE REFERENCE: the analysis direction of the vocoder goldens.

Like ``make_golden.py`` this runs only where the reference tree is importable; the fixture it writes is plain data and is
committed, so the tests never need the reference.  The models of ``squeezewave_{small,full}.npz`` are rebuilt from those
fixtures (nothing is overwritten), put in eval mode, and the reference's own ``SqueezeWave.forward``
(``squeeze_wave/modules.py:294-332``) and ``SqueezeWaveLoss(1.0)`` (``squeeze_wave/loss.py:14-31``) are run on each
golden's own ``mel`` and ``audio``.  Per tag the fixture holds

  <tag>/z          the latent (B, n_audio_channels, L), fp32
  <tag>/loss       SqueezeWaveLoss(1.0) of the whole batch
  <tag>/log_s_sum  sum of log_s per flow (float64 sum of the reference's fp32 tensor)
  <tag>/log_det_W  the reference's log_det_W per flow (B * L * logdet W)
  <tag>/ragged     the loss of each piece of the ragged split -- frames [7, 0, 17] of utterance 0, consecutive -- scored
                   ALONE by the reference (NaN for the empty piece: there is nothing to score)

The archive is written with fixed member timestamps and one thread computes it, so it regenerates bit for bit.

    python tests/golden/make_likelihood_golden.py
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("RTTS_REFERENCE", "/root/reference"))

import sw_likelihood_ref as ref64  # noqa: E402


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the current time: the bytes would differ per run)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    sys.modules.setdefault("dacite", types.ModuleType("dacite"))
    from reformer_tts.squeeze_wave.config import WNConfig
    from reformer_tts.squeeze_wave.loss import SqueezeWaveLoss
    from reformer_tts.squeeze_wave.modules import SqueezeWave
    torch.set_num_threads(1)
    out = {}
    for tag in ("small", "full"):
        cfg, sd, mel, audio = ref64.load_case(HERE, tag)
        wn = cfg["wn_config"]
        m = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                        cfg["early_return_size"], WNConfig(wn["n_layers"], wn["n_channels"], wn["conv_kernel_size"], wn["mel_upsample_scale"]))
        missing = m.load_state_dict(sd, strict=False)
        assert not missing.unexpected_keys and all("num_batches" in k for k in missing.missing_keys), missing
        m.eval()
        loss = SqueezeWaveLoss(1.0)
        with torch.no_grad():
            z, log_s_list, log_det_list = m.forward((mel, audio))
            out[f"{tag}/z"] = z.numpy().astype(np.float32)
            out[f"{tag}/loss"] = np.array(float(loss((z, log_s_list, log_det_list))), dtype=np.float32)
            out[f"{tag}/log_s_sum"] = np.array([float(s.double().sum()) for s in log_s_list], dtype=np.float64)
            out[f"{tag}/log_det_W"] = np.array([float(d) for d in log_det_list], dtype=np.float32)
            pieces = []
            for pmel, paudio in ref64.ragged_pieces(mel, audio):
                pieces.append(float(loss(m.forward((pmel, paudio)))) if pmel.shape[2] else float("nan"))
            out[f"{tag}/ragged"] = np.array(pieces, dtype=np.float32)
        out[f"{tag}/ragged_frames"] = np.array(ref64.RAGGED_FRAMES, dtype=np.int64)
        print(tag, "z", tuple(z.shape), "loss", out[f"{tag}/loss"], "max |log_s|", max(float(s.abs().max()) for s in log_s_list),
              "ragged", out[f"{tag}/ragged"])
    path = os.path.join(HERE, "squeezewave_likelihood.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
