"""float64 restatement of one SqueezeWave TRAINING step -- TEST HELPER, not the product (like tests/sw_likelihood_ref.py).

``forward64`` / ``loss64`` of ``sw_likelihood_ref`` with the BatchNorms in training mode (``F.batch_norm(..., training=True)``:
batch statistics over the B * L rows, reference ``squeeze_wave/modules.py:100-117``), made differentiable: the leaves are
float64 copies of the state dict with ``requires_grad`` (running statistics excluded), the gradients come from autograd.

``rounded=True`` is the ROUNDING MODEL of the HIP executor, as in ``sw_likelihood_ref``: the same arithmetic rounded to bf16
wherever the executor holds a bf16 value.  Autograd through the bf16 casts rounds the gradients at the same places.  The model
says nothing about accumulation order or the device's ``exp`` / ``tanh``: the GPU tests take 4x its error as their bound.

Cases (built from the committed goldens only):
    small       squeezewave_small.npz as is                     B 2, Lm 24, up 16   toy widths (library GEMM path)
    full/3x10   frames [0,10), [10,20), [20,30) of the one      60 rows, up 2       in-tree; the 128-row padding and M % 64
                ``full`` utterance as three utterances
    full/2x16   frames [0,16), [16,32) likewise                 64 rows, up 2       in-tree; a row count that tiles exactly"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

import sw_likelihood_ref as ref64
from sw_likelihood_ref import SD, bf16

CASES = ("small", "full/3x10", "full/2x16")
_SPLIT = {"full/3x10": (3, 10), "full/2x16": (2, 16)}
LEARNING_RATE = 4e-4

# Per case, the bf16 rounding model against the exact float64 step, as ``model_constants`` measures them
# (tests/test_sw_train_cpu.py re-measures and compares; the GPU tests allow 4x):
#   (worst per-tensor relative L2 gradient error, relative L2 error of all gradients concatenated, |loss difference|,
#    worst per-step |loss difference| of ``train64`` over 8 steps, worst relative L2 error of a BatchNorm's updated running_mean,
#    the same for running_var)
MODEL_CONST: Dict[str, Tuple[float, float, float, float, float, float]] = {
    "small": (1.264e-2, 2.903e-3, 8.759e-5, 8.759e-5, 1.022e-3, 1.722e-4),
    "full/3x10": (1.549e-2, 3.704e-3, 2.264e-5, 8.489e-5, 2.048e-3, 3.067e-4),
    "full/2x16": (1.399e-2, 3.690e-3, 2.385e-5, 3.970e-4, 2.043e-3, 2.953e-4),
}


def load_train_case(golden_dir: str, name: str):
    """-> (cfg, fp32 state dict, mel (B, n_mel, Lm), audio (B, 256 * Lm)) of a training case."""
    cfg, sd, mel, audio = ref64.load_case(golden_dir, name.split("/")[0])
    if name in _SPLIT:
        nb, f = _SPLIT[name]
        assert mel.shape[2] >= nb * f, (name, mel.shape)
        mel = torch.cat([mel[:1, :, i * f:(i + 1) * f] for i in range(nb)]).contiguous()
        audio = torch.cat([audio[:1, 256 * i * f:256 * (i + 1) * f] for i in range(nb)]).contiguous()
    return cfg, sd, mel, audio


def is_stat(name: str) -> bool:
    return name.endswith(("running_mean", "running_var", "num_batches_tracked"))


def leaves64(sd: SD) -> SD:
    """float64 leaves with requires_grad for every parameter; the running statistics as plain float64 copies."""
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        out[k] = v.detach().double().clone()
        if not is_stat(k):
            out[k].requires_grad_(True)
    return out


def wn64_train(sd: SD, p: str, a0: torch.Tensor, mel: torch.Tensor, wn: dict, rounded: bool) -> torch.Tensor:
    """``sw_likelihood_ref.wn64`` with batch-statistics BatchNorm; the running statistics in ``sd`` are updated in place
    (momentum 0.1, unbiased variance), as ``nn.BatchNorm1d`` does in ``.train()``."""
    c, nl = wn["n_channels"], wn["n_layers"]
    r = bf16 if rounded else (lambda t: t)
    in_tree = c % 64 == 0 and a0.shape[1] % 8 == 0 and mel.shape[1] % 8 == 0
    b = lambda k: sd[p + k]        # noqa: E731
    w = lambda q: ref64._weight(sd, q)        # noqa: E731
    h = F.conv1d(r(a0) if in_tree else a0, r(w(p + "start_conv.")), b("start_conv.bias"))
    cond = r(F.conv1d(r(mel), r(w(p + "cond_layer.")), b("cond_layer.bias") if in_tree else r(b("cond_layer.bias"))))
    for i in range(nl):
        spec = cond[:, i * 2 * c:(i + 1) * 2 * c, :]
        if h.shape[2] > spec.shape[2]:
            spec = spec.repeat_interleave(wn["mel_upsample_scale"], dim=2)
        q = f"in_layers.{i}.layer."
        x = F.batch_norm(h, b(q + "0.running_mean"), b(q + "0.running_var"), b(q + "0.weight"), b(q + "0.bias"), True, 0.1, 1e-5)
        x = r(F.conv1d(x, b(q + "1.weight"), b(q + "1.bias"), padding=(wn["conv_kernel_size"] - 1) // 2, groups=c))
        pw = r(F.conv1d(x, r(b(q + "2.weight")), b(q + "2.bias")))
        s = pw + spec
        acts = r(torch.tanh(s[:, :c]) * torch.sigmoid(s[:, c:]))
        rs = r(F.conv1d(acts, r(w(p + f"res_skip_layers.{i}."))))
        h = h + rs + b(f"res_skip_layers.{i}.bias").view(1, -1, 1)
    return F.conv1d(r(h), r(b("end_conv.weight")), b("end_conv.bias"))


def forward64_train(sd: SD, cfg: dict, mel: torch.Tensor, audio: torch.Tensor, rounded: bool = False):
    """``sw_likelihood_ref.forward64`` in training mode, differentiable in the entries of ``sd`` (float64)."""
    c = cfg["n_audio_channels"]
    mel, audio = mel.double(), audio.double()
    audio = audio.unfold(1, c, c).permute(0, 2, 1)
    outs, log_s_list, log_det_list = [], [], []
    for k in range(cfg["n_flows"]):
        if ref64._return_early(cfg, k):
            outs.append(audio[:, :cfg["early_return_size"]])
            audio = audio[:, cfg["early_return_size"]:]
        w = sd[f"inv_conv_layers.{k}.conv.weight"].squeeze(-1)
        sign, logabs = torch.linalg.slogdet(w)
        assert sign > 0, k
        log_det_list.append(audio.shape[0] * audio.shape[2] * logabs)
        audio = F.conv1d(audio, w.unsqueeze(-1))
        half = audio.shape[1] // 2
        a0, a1 = audio[:, :half], audio[:, half:]
        out = wn64_train(sd, f"wn_layers.{k}.", a0, mel, cfg["wn_config"], rounded)
        log_s, bb = out[:, :half], out[:, half:]
        audio = torch.cat([a0, torch.exp(log_s) * a1 + bb], 1)
        log_s_list.append(log_s)
    outs.append(audio)
    return torch.cat(outs, 1), log_s_list, log_det_list


def step64(leaves: SD, cfg: dict, mel, audio, rounded: bool, sigma: float = 1.0) -> torch.Tensor:
    """One forward + backward on ``leaves`` (gradients ADD into ``.grad``, running statistics updated) -> the loss (0-dim)."""
    loss = ref64.loss64(forward64_train(leaves, cfg, mel, audio, rounded), sigma)
    loss.backward()
    return loss.detach()


_CACHE: dict = {}


def grads64(golden_dir: str, name: str, rounded: bool):
    """-> (loss (float), {parameter: float64 gradient}, {running statistic: float64 value after the step}); computed once."""
    key = ("grads", name, rounded)
    if key not in _CACHE:
        cfg, sd, mel, audio = load_train_case(golden_dir, name)
        leaves = leaves64(sd)
        loss = float(step64(leaves, cfg, mel, audio, rounded))
        grads = {k: v.grad.detach().clone() for k, v in leaves.items() if not is_stat(k)}
        stats = {k: v.detach().clone() for k, v in leaves.items() if is_stat(k)}
        _CACHE[key] = (loss, grads, stats)
    return _CACHE[key]


def train64(golden_dir: str, name: str, steps: int, rounded: bool) -> List[float]:
    """``steps`` steps of ``torch.optim.Adam(lr=4e-4)`` on one fixed batch -> the loss of every step; computed once."""
    key = ("train", name, steps, rounded)
    if key not in _CACHE:
        cfg, sd, mel, audio = load_train_case(golden_dir, name)
        leaves = leaves64(sd)
        opt = torch.optim.Adam([v for k, v in leaves.items() if not is_stat(k)], lr=LEARNING_RATE)
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            losses.append(float(step64(leaves, cfg, mel, audio, rounded)))
            opt.step()
        _CACHE[key] = losses
    return _CACHE[key]


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    return float((got.double().reshape(-1) - want.double().reshape(-1)).norm() / want.double().norm())


def concat_rel_l2(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor]) -> float:
    num = sum(float((got[k].double().reshape(-1) - want[k].double().reshape(-1)).pow(2).sum()) for k in want)
    den = sum(float(want[k].double().pow(2).sum()) for k in want)
    return (num / den) ** 0.5


def model_constants(golden_dir: str, name: str, steps: int = 8) -> Tuple[float, float, float, float, float, float]:
    """What ``MODEL_CONST[name]`` records, measured."""
    le, ge, se = grads64(golden_dir, name, False)
    lm, gm, sm = grads64(golden_dir, name, True)
    worst = max(rel_l2(gm[k], ge[k]) for k in ge)
    te, tm = train64(golden_dir, name, steps, False), train64(golden_dir, name, steps, True)
    rm = max(rel_l2(sm[k], se[k]) for k in se if k.endswith("running_mean"))
    rv = max(rel_l2(sm[k], se[k]) for k in se if k.endswith("running_var"))
    return worst, concat_rel_l2(gm, ge), abs(le - lm), max(abs(a - b) for a, b in zip(te, tm)), rm, rv
