#!/usr/bin/env python3
"""Generate ``alignment_small.npz`` FROM THE REFERENCE: the decoder's encoder-decoder attention matrices of an eval-mode,
teacher-forced forward, called the way ``validation_step`` calls it (``training/wrappers.py:107-128``: ``spectrogram[:, :-1]``,
``spectrogram_mask = loss_mask.mean(-1)``).

Runs only in the build container (needs the reference checkout, ``REFERENCE_ROOT``, default ``/root/reference``); the fixture is
plain data and is committed, so the tests never need the reference.  Set up like ``make_golden.py``: the reference's own
``ReformerTTS`` with ``reformer_pytorch`` (absent here) replaced by ``oracle.lsh_ref.LSHSelfAttention``, parameters from
``oracle.synth`` (shapes stored, values not), non-trivial BatchNorm running statistics (stored), and every LSH rotation
recorded in call order.

    python tests/golden/make_alignment_golden.py

Fixture
  alignment_small.npz  ``oracle.model_ref.small_cfg()`` (d = 128, 2 heads of dh = 64, pad_base 128) with decoder depth 2;
                       B = 2, ragged text up to 150 phonemes (padded to 256 keys: two key chunks) and mel up to 120 frames
                       (padded to 128 queries).  ``att/<layer>``: the (B, T_q padded, T_k padded) head-averaged weights as
                       float16 (values in [0, 1]: absolute rounding <= 2.5e-4).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get("REFERENCE_ROOT", "/root/reference"))

from oracle import lsh_ref, model_ref, synth  # noqa: E402

shim = types.ModuleType("reformer_pytorch")
shim.LSHSelfAttention = lsh_ref.LSHSelfAttention
sys.modules["reformer_pytorch"] = shim

from reformer_tts.model.reformer_tts import ReformerTTS  # noqa: E402


def npy(t):
    return t.detach().cpu().numpy()


def alignment_small():
    cfg = model_ref.small_cfg()
    cfg["dec_reformer_kwargs"]["depth"] = 2
    torch.manual_seed(7)
    m = ReformerTTS(**cfg)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(synth.synth_state_dict(shapes, seed=3), strict=False)
    g = torch.Generator().manual_seed(31)
    out = {f"shape/{k}": np.array(s, dtype=np.int64) for k, s in shapes.items()}
    for name, buf in m.named_buffers():
        if name.endswith("running_mean"):
            buf.copy_(0.2 * torch.randn(buf.shape, generator=g))
        elif name.endswith("running_var"):
            buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
        if "running" in name:
            out[f"buf/{name}"] = npy(buf)
    batch = model_ref.synthetic_batch(2, 150, 120, ragged=True, seed=9)
    for k, v in batch.items():
        out[f"batch/{k}"] = npy(v)
    rot_log = []
    for mod in m.modules():
        if isinstance(mod, lsh_ref.LSHSelfAttention):
            mod.rotation_log = rot_log
    m.eval()
    spec = batch["spectrogram"]
    torch.manual_seed(11)
    with torch.no_grad():
        raw, post, stop, mats = m(batch["phonemes"], spec[:, :-1], batch["loss_mask"].mean(-1))
    assert len(mats) == cfg["dec_reformer_kwargs"]["depth"], len(mats)
    for i, r in enumerate(rot_log):
        out[f"rot/{i}"] = npy(r)
    out["n_rot"] = np.array(len(rot_log))
    for i, a in enumerate(mats):
        out[f"att/{i}"] = npy(a).astype(np.float16)
    out["out/post"] = npy(post).astype(np.float16)
    np.savez_compressed(os.path.join(HERE, "alignment_small.npz"), **out)
    print("alignment_small.npz: layers", len(mats), "matrix", tuple(mats[0].shape), "text lengths",
          npy((batch["phonemes"] != 0).sum(1)).tolist(), "rotations", [tuple(r.shape) for r in rot_log],
          "bytes", os.path.getsize(os.path.join(HERE, "alignment_small.npz")))


if __name__ == "__main__":
    alignment_small()
