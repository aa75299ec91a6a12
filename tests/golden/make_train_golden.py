#!/usr/bin/env python3
"""Generate ``squeezewave_train.npz`` FROM THE REFERENCE: one training-mode forward + backward of the vocoder.

Like ``make_likelihood_golden.py`` this runs only where the reference tree is importable; the fixture it writes is plain data
and is committed, so the tests never need the reference.  For each case of ``tests/sw_train_ref.py`` (``small``,
``full/3x10``, ``full/2x16``: built from ``squeezewave_{small,full}.npz``, nothing is overwritten) the reference's own
``SqueezeWave`` is put in ``.train()``, ``SqueezeWaveLoss(1.0)(model((mel, audio)))`` is back-propagated once (what
``LitSqueezeWave.training_step``, ``training/wrappers.py:350-359``, hands to the optimiser), and the fixture holds

  <case>/loss                 the loss
  <case>/names                every parameter's name, in ``named_parameters`` order
  <case>/norms                the L2 norm of every parameter's gradient (float64 norm of the reference's fp32 gradient), same order
  <case>/grad/<name>          in full, the gradients of wn_layers.0.in_layers.0.layer.{0,1}.*, wn_layers.0.cond_layer.weight_g
                              and inv_conv_layers.{0,2}.conv.weight
  <case>/stat/<name>          running_mean, running_var, num_batches_tracked of wn_layers.0.in_layers.0.layer.0 after the step

The archive is written with fixed member timestamps and one thread computes it, so it regenerates bit for bit.

    python tests/golden/make_train_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get("RTTS_REFERENCE", "/root/reference"))

import sw_train_ref as train64  # noqa: E402
from make_likelihood_golden import save_npz  # noqa: E402

FULL = ("wn_layers.0.in_layers.0.layer.0.", "wn_layers.0.in_layers.0.layer.1.", "wn_layers.0.cond_layer.weight_g",
        "inv_conv_layers.0.conv.weight", "inv_conv_layers.2.conv.weight")
STATS = "wn_layers.0.in_layers.0.layer.0."


def main():
    sys.modules.setdefault("dacite", types.ModuleType("dacite"))
    from reformer_tts.squeeze_wave.config import WNConfig
    from reformer_tts.squeeze_wave.loss import SqueezeWaveLoss
    from reformer_tts.squeeze_wave.modules import SqueezeWave
    torch.set_num_threads(1)
    out = {}
    for case in train64.CASES:
        cfg, sd, mel, audio = train64.load_train_case(HERE, case)
        wn = cfg["wn_config"]
        m = SqueezeWave(cfg["n_flows"], cfg["n_audio_channels"], cfg["n_mel_channels"], cfg["early_return_interval"],
                        cfg["early_return_size"], WNConfig(wn["n_layers"], wn["n_channels"], wn["conv_kernel_size"], wn["mel_upsample_scale"]))
        missing = m.load_state_dict(sd, strict=False)
        assert not missing.unexpected_keys and all("num_batches" in k for k in missing.missing_keys), missing
        m.train()
        loss = SqueezeWaveLoss(1.0)(m((mel, audio)))
        loss.backward()
        names = [n for n, _ in m.named_parameters()]
        assert all(p.grad is not None for p in m.parameters())
        out[f"{case}/loss"] = np.array(float(loss), dtype=np.float32)
        out[f"{case}/names"] = np.array(names)
        out[f"{case}/norms"] = np.array([float(p.grad.double().norm()) for p in m.parameters()], dtype=np.float64)
        for n, p in m.named_parameters():
            if n.startswith(FULL):
                out[f"{case}/grad/{n}"] = p.grad.numpy().astype(np.float32)
        for n, b in m.named_buffers():
            if n.startswith(STATS):
                out[f"{case}/stat/{n}"] = b.detach().numpy().copy()
        print(case, "loss", out[f"{case}/loss"], "parameters", len(names), "smallest gradient norm", out[f"{case}/norms"].min())
    path = os.path.join(HERE, "squeezewave_train.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
