"""CPU side of the attention-alignment surface: the validation trimming helper against a restatement of the reference's
(training/wrappers.py:316-325), and the C declaration of the probability kernel against its ctypes binding."""
import inspect
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_trim(attention_matrices, stop_tokens):
    """``LitReformerTTS.trim_attention_matrices`` (training/wrappers.py:316-325), restated."""
    stop_indexes = stop_tokens.argmax(dim=1)
    result = []
    for i, stop_index in enumerate(stop_indexes):
        result.append([matrix[i, :stop_index, :] for matrix in attention_matrices])
    return result


def test_trim_attention_matrices_matches_the_reference():
    from reformer_tts_amd.training import trim_attention_matrices
    g = torch.Generator().manual_seed(0)
    b, t, tk = 4, 30, 16
    mats = [torch.rand(b, t, tk, generator=g) for _ in range(3)]
    stop = torch.zeros(b, t)
    for i, s in enumerate((29, 0, 7, 12)):
        stop[i, s] = 1.0
    stop[3, 20] = 1.0                                      # two ones: argmax takes the first, as in the reference
    got, want = trim_attention_matrices(mats, stop), _reference_trim(mats, stop)
    assert len(got) == len(want) == b
    for per_got, per_want in zip(got, want):
        assert len(per_got) == len(per_want) == len(mats)
        for x, y in zip(per_got, per_want):
            assert x.shape == y.shape and torch.equal(x, y)
    assert [m.shape[0] for m in (p[0] for p in got)] == [29, 0, 7, 12]
    assert trim_attention_matrices([], stop) == [[] for _ in range(b)]


def test_alignment_switches_default_to_the_reference_behaviour():
    """Eval forwards collect by default (as the reference); validate() returns the five scalars unless asked for more."""
    from reformer_tts_amd.model.reformer import ReformerDec
    from reformer_tts_amd.training import Trainer
    assert ReformerDec.collect_attention is True
    assert inspect.signature(Trainer.validate).parameters["return_attention"].default is False


def test_probs_mean_declaration_matches_the_binding():
    from reformer_tts_amd import _lib
    text = open(os.path.join(ROOT, "include", "rtts.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int rtts_xattn_probs_mean\(([^)]*)\);", text)
    assert m, "rtts_xattn_probs_mean is not declared in include/rtts.h"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES["rtts_xattn_probs_mean"]) == 14
