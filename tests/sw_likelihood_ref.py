"""float64 restatement of the SqueezeWave likelihood -- TEST HELPER, not the product (like tests/mel_ref.py).

``forward64`` follows ``SqueezeWave.forward`` (reference ``squeeze_wave/modules.py:294-332``, ``WN.forward`` :203-235,
``InvertibleConv1d.forward`` :53-65) functionally over a reference-named ``state_dict`` with the BatchNorms in eval mode, in
float64; ``loss64`` is ``SqueezeWaveLoss`` (``squeeze_wave/loss.py:14-31``).

``forward64(..., rounded=True)`` is a ROUNDING MODEL of the HIP executor (``reformer_tts_amd/squeeze_wave/modules.py``): the
same float64 arithmetic, rounded to bf16 wherever the executor holds a bf16 value -- both operands of every 1x1-convolution
GEMM and every bf16 buffer (the mel conditioning, the depthwise output, the pointwise output, the gate output, the
residual/skip product, and the residual stream in front of ``end_conv``).  The audio path (coupling, invertible 1x1
convolution, z) and the residual stream itself stay unrounded, as they are fp32 there.  The model says nothing about
accumulation order or the device's ``exp`` / ``tanh``: the tests take 4x its error as their bound.  For the toy widths that
the MFMA GEMM does not tile (``_FoldedWN.in_tree`` False) the executor keeps the ``start_conv`` input in fp32 and adds the
conditioning bias in bf16; the model follows it."""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

SD = Dict[str, torch.Tensor]

RAGGED_FRAMES = [7, 0, 17]          # the fixture's ragged split: consecutive pieces of utterance 0

# (max |z err|, mean |z err|, |loss diff|) of the bf16 rounding model against the float64 forward on the golden inputs, as
# ``rounding_model_error`` measures them (tests/test_sw_likelihood_cpu.py re-measures and compares); the GPU tests allow 4x.
MODEL_ERR = {"small": (5.852e-3, 7.983e-4, 6.671e-5), "full": (5.212e-3, 8.648e-4, 1.672e-5)}


def small_cfg() -> dict:
    return dict(n_mel_channels=80, n_flows=4, n_audio_channels=16, early_return_interval=2, early_return_size=4,
                wn_config=dict(n_layers=2, n_channels=32, conv_kernel_size=3, mel_upsample_scale=16))


def default_cfg() -> dict:
    return dict(n_mel_channels=80, n_flows=12, n_audio_channels=128, early_return_interval=2, early_return_size=16,
                wn_config=dict(n_layers=8, n_channels=256, conv_kernel_size=3, mel_upsample_scale=2))


def cfg_of(tag: str) -> dict:
    return small_cfg() if tag == "small" else default_cfg()


def load_case(golden_dir: str, tag: str) -> Tuple[dict, SD, torch.Tensor, torch.Tensor]:
    """-> (cfg, fp32 state dict, mel, audio) of the vocoder golden ``squeezewave_<tag>.npz``: 'small' stores its whole state
    dict, 'full' its BatchNorm statistics and 1x1 weights over a seeded synthetic one (as tests/test_squeezewave_hip.py)."""
    from oracle import synth
    z = np.load(os.path.join(golden_dir, f"squeezewave_{tag}.npz"))
    if tag == "small":
        sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    else:
        shapes = {k[len("shape/"):]: tuple(z[k]) for k in z.files if k.startswith("shape/")}
        sd = {k: v * (0.05 if "end_conv" in k else 1.0) for k, v in synth.synth_state_dict(shapes, seed=11).items()}
        for k in z.files:
            if k.startswith("sd/"):
                sd[k[3:]] = torch.from_numpy(z[k])
    return cfg_of(tag), sd, torch.from_numpy(z["mel"]), torch.from_numpy(z["audio"])


def bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to the nearest bf16 value (ties to even), kept in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _weight(sd: SD, p: str) -> torch.Tensor:
    if p + "weight" in sd:
        return sd[p + "weight"].double()
    v, g = sd[p + "weight_v"].double(), sd[p + "weight_g"].double()
    return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))


def _return_early(cfg: dict, k: int) -> bool:
    return k % cfg["early_return_interval"] == 0 and k > 0


def wn64(sd: SD, p: str, a0: torch.Tensor, mel: torch.Tensor, wn: dict, rounded: bool) -> torch.Tensor:
    """``WN.forward`` in float64: a0 (B, n_half, L), mel (B, n_mel, Lm) -> (B, 2 * n_half, L)."""
    c, nl = wn["n_channels"], wn["n_layers"]
    r = bf16 if rounded else (lambda t: t)
    in_tree = c % 64 == 0 and a0.shape[1] % 8 == 0 and mel.shape[1] % 8 == 0
    b = lambda k: sd[p + k].double()        # noqa: E731
    h = F.conv1d(r(a0) if in_tree else a0, r(_weight(sd, p + "start_conv.")), b("start_conv.bias"))
    cond = r(F.conv1d(r(mel), r(_weight(sd, p + "cond_layer.")), b("cond_layer.bias") if in_tree else r(b("cond_layer.bias"))))
    for i in range(nl):
        spec = cond[:, i * 2 * c:(i + 1) * 2 * c, :]
        if h.shape[2] > spec.shape[2]:
            spec = spec.repeat_interleave(wn["mel_upsample_scale"], dim=2)
        q = f"in_layers.{i}.layer."
        x = F.batch_norm(h, b(q + "0.running_mean"), b(q + "0.running_var"), b(q + "0.weight"), b(q + "0.bias"), False, 0.1, 1e-5)
        x = r(F.conv1d(x, b(q + "1.weight"), b(q + "1.bias"), padding=(wn["conv_kernel_size"] - 1) // 2, groups=c))
        pw = r(F.conv1d(x, r(b(q + "2.weight")), b(q + "2.bias")))
        s = pw + spec
        acts = r(torch.tanh(s[:, :c]) * torch.sigmoid(s[:, c:]))
        rs = r(F.conv1d(acts, r(_weight(sd, p + f"res_skip_layers.{i}."))))
        h = h + rs + b(f"res_skip_layers.{i}.bias").view(1, -1, 1)
    return F.conv1d(r(h), r(b("end_conv.weight")), b("end_conv.bias"))


def forward64(sd: SD, cfg: dict, mel: torch.Tensor, audio: torch.Tensor, rounded: bool = False):
    """``SqueezeWave.forward``: mel (B, n_mel, Lm), audio (B, 256 * Lm) -> (z (B, C, L), log_s_list, log_det_W_list), all
    float64; ``log_det_W_list[k]`` = B * L * log det W_k (0-dim)."""
    c = cfg["n_audio_channels"]
    mel, audio = mel.double(), audio.double()
    audio = audio.unfold(1, c, c).permute(0, 2, 1)
    outs, log_s_list, log_det_list = [], [], []
    for k in range(cfg["n_flows"]):
        if _return_early(cfg, k):
            outs.append(audio[:, :cfg["early_return_size"]])
            audio = audio[:, cfg["early_return_size"]:]
        w = sd[f"inv_conv_layers.{k}.conv.weight"].double().squeeze(-1)
        sign, logabs = torch.linalg.slogdet(w)
        assert sign > 0, k
        log_det_list.append(audio.shape[0] * audio.shape[2] * logabs)
        audio = F.conv1d(audio, w.unsqueeze(-1))
        half = audio.shape[1] // 2
        a0, a1 = audio[:, :half], audio[:, half:]
        out = wn64(sd, f"wn_layers.{k}.", a0, mel, cfg["wn_config"], rounded)
        log_s, bb = out[:, :half], out[:, half:]
        audio = torch.cat([a0, torch.exp(log_s) * a1 + bb], 1)
        log_s_list.append(log_s)
    outs.append(audio)
    return torch.cat(outs, 1), log_s_list, log_det_list


def loss64(output, sigma: float = 1.0) -> torch.Tensor:
    """``SqueezeWaveLoss(sigma)`` in float64 (0-dim)."""
    z, log_s_list, log_det_list = output
    total = torch.sum(z.double() ** 2) / (2.0 * sigma ** 2)
    for log_s, ld in zip(log_s_list, log_det_list):
        total = total - log_s.double().sum() - torch.as_tensor(ld).double()
    return total / z.numel()


def ragged_pieces(mel: torch.Tensor, audio: torch.Tensor, frames: List[int] = RAGGED_FRAMES, spf: int = 256):
    """Consecutive pieces of utterance 0: [(mel (1, n_mel, f), audio (1, spf * f))] for f in ``frames``."""
    out, t = [], 0
    for f in frames:
        out.append((mel[:1, :, t:t + f], audio[:1, spf * t:spf * (t + f)]))
        t += f
    return out


def rounding_model_error(golden_dir: str, tag: str) -> Tuple[float, float, float]:
    """(max |z err|, mean |z err|, |loss diff|) of the bf16 rounding model against the float64 forward on the golden inputs."""
    cfg, sd, mel, audio = load_case(golden_dir, tag)
    exact = forward64(sd, cfg, mel, audio)
    model = forward64(sd, cfg, mel, audio, rounded=True)
    err = (exact[0] - model[0]).abs()
    return float(err.max()), float(err.mean()), abs(float(loss64(exact) - loss64(model)))
