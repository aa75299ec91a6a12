"""``rtts_tts_collate`` on the GPU, bit for bit against the reference's collate and against what the host path puts into a captured
step's buffers.

A toy corpus of seven utterances (tests/tts_corpus_ref.py: mel lengths 1, 2, 63, 64, 65, 130, 64 so that columns start at odd
element offsets and a batch spans one to three 64-row tiles; sentinel columns and ids behind the data), every output prefilled with
NaN / -1 so that a word the launch does not write shows.  The input noise against Box-Muller in float64 from the same hash words."""
import numpy as np
import pytest
import torch

import tts_corpus_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7.0e9
CASES = ([5], [0, 0, 3], [6, 5, 4, 2, 1])


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class _Toy:
    def __init__(self, gpu, n_mel):
        from reformer_tts_amd.dataset import TTSCorpus
        self.items, self.n_mel, self.gpu = ref.toy_items(n_mel), n_mel, gpu
        mel = torch.cat([e["spectrogram"].t() for e in self.items] + [torch.full((n_mel, 5), SENTINEL)], dim=1).contiguous()
        ph = torch.cat([e["phonemes"] for e in self.items] + [torch.full((3,), 999)]).to(torch.int32)
        fo, po = np.cumsum((0,) + ref.MEL_LENGTHS).tolist(), np.cumsum((0,) + ref.PHONEME_LENGTHS).tolist()
        self.corpus = TTSCorpus(mel.to(gpu), fo, ph.to(gpu), po)

    def outputs(self, b, LP, R_in, R):
        nan, g = float("nan"), self.gpu
        return dict(phonemes=torch.full((b, LP), -1, dtype=torch.int64, device=g), spectrogram_input=torch.full((b, R_in, self.n_mel), nan, device=g),
                    spectrogram_target=torch.full((b, R, self.n_mel), nan, device=g), stop_tokens=torch.full((b, R), nan, device=g),
                    loss_mask=torch.full((b, R, self.n_mel), nan, device=g), valid_len=torch.full((1,), -1, dtype=torch.int32, device=g))

    def launch(self, ids, lm, out, tables=None, **kw):
        from reformer_tts_amd import ops
        c = self.corpus
        fo, po = c.tables if tables is None else tables
        ops.tts_collate(c.mel, fo, c.phoneme_ids, po, torch.tensor(ids, dtype=torch.int32, device=self.gpu), lm, **out, **kw)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}

    def shape(self, ids):
        return max(ref.PHONEME_LENGTHS[i] for i in ids), max(ref.MEL_LENGTHS[i] for i in ids)


@pytest.fixture(scope="module", params=[80, 8, 128])
def toy(request, gpu):
    return _Toy(gpu, request.param)


def _same(got, want, keys=None):
    for k in keys or want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------ 1. the reference's layout
@pytest.mark.parametrize("ids", CASES, ids=str)
def test_reference_layout_is_custom_sequence_padder(toy, ids):
    from reformer_tts_amd.dataset import custom_sequence_padder
    pad = custom_sequence_padder([toy.items[i] for i in ids])
    lp, lm = toy.shape(ids)
    got = toy.launch(ids, lm, toy.outputs(len(ids), lp, lm + 1, lm))
    want = dict(phonemes=pad["phonemes"], spectrogram_input=pad["spectrogram"], spectrogram_target=pad["spectrogram"][:, 1:],
                stop_tokens=pad["stop_tokens"], loss_mask=pad["loss_mask"], valid_len=torch.tensor([lm], dtype=torch.int32))
    _same(got, want)
    batch = toy.corpus.collate(ids)
    torch.cuda.synchronize()
    assert sorted(batch) == sorted(pad)
    _same({k: v.cpu() for k, v in batch.items()}, pad)


# ------------------------------------------------------------------ 2. the buffers of a captured step
@pytest.mark.parametrize("ids", CASES, ids=str)
def test_graph_layout_is_fill_shape_buffers(toy, ids, gpu):
    from reformer_tts_amd.dataset import custom_sequence_padder
    from reformer_tts_amd.training import Trainer
    pad = {k: v.to(gpu) for k, v in custom_sequence_padder([toy.items[i] for i in ids]).items()}
    lp, lm = toy.shape(ids)
    for LM in (lm, -(-lm // 128) * 128):
        LP = -(-lp // 128) * 128
        want = toy.outputs(len(ids), LP, LM, LM)
        Trainer._fill_shape_buffers(None, dict(bufs=want), pad)
        got = toy.outputs(len(ids), LP, LM, LM)
        toy.corpus.fill(got, ids)
        torch.cuda.synchronize()
        _same({k: v.cpu() for k, v in got.items()}, {k: v.cpu() for k, v in want.items()})
        assert int(got["valid_len"]) == lm
        again = toy.outputs(len(ids), LP, LM, LM)                                   # ids already on the device: a slice of a plan
        plan = torch.tensor([3] + list(ids) + [1], dtype=torch.int32, device=gpu)
        toy.corpus.fill(again, plan[1:1 + len(ids)], lm=lm)
        torch.cuda.synchronize()
        _same({k: v.cpu() for k, v in again.items()}, {k: v.cpu() for k, v in want.items()})
    assert ref.collate([toy.items[i] for i in ids], toy.n_mel, LP=LP, R_in=LM, valid_in=lm, R=LM)["spectrogram_input"].equal(got["spectrogram_input"].cpu())


# ------------------------------------------------------------------ 3. utterances that do not exist
def test_strangers_are_all_zero_slots(toy, gpu):
    it = toy.items
    for ids, present in (([1, 7, 3], [it[1], None, it[3]]), ([-1], [None]), ([2, -2147483648, 2147483647, 0], [it[2], None, None, it[0]])):
        real = [i for i in ids if 0 <= i < 7]
        lp, lm = toy.shape(real) if real else (4, 4)
        got = toy.launch(ids, lm, toy.outputs(len(ids), lp, lm + 1, lm))
        want = ref.collate(present, toy.n_mel, LP=lp, R_in=lm + 1, valid_in=lm + 1, R=lm)
        _same(got, want)
    # offset tables that decrease or point outside the buffers: the utterance does not exist, nothing is read
    fo, po = (t.clone() for t in toy.corpus.tables)
    bad_fo, bad_po, bad_dec = fo.clone(), po.clone(), fo.clone()
    bad_fo[-1] = toy.corpus.mel.shape[1] + 1                                         # utterance 6 ends outside mel
    bad_po[-1] = toy.corpus.phoneme_ids.numel() + 1                                  # utterance 6's ids end outside the buffer
    bad_dec[3] = bad_dec[2] - 1                                                      # utterance 2 ends in front of its start (and 3 starts there)
    for tables, gone in (((bad_fo, po), {6}), ((fo, bad_po), {6}), ((bad_dec, po), {2})):
        ids = [6, 2, 0]
        lp, lm = toy.shape(ids)
        got = toy.launch(ids, lm, toy.outputs(3, lp, lm + 1, lm), tables=tables)
        want = ref.collate([None if i in gone else it[i] for i in ids], toy.n_mel, LP=lp, R_in=lm + 1, valid_in=lm + 1, R=lm)
        _same(got, want)
    with pytest.raises(IndexError):
        toy.corpus.collate([1, 7])


# ------------------------------------------------------------------ 4. null outputs
def test_null_outputs_are_skipped(toy):
    ids = [6, 5, 4, 2, 1]
    lp, lm = toy.shape(ids)
    full = toy.launch(ids, lm, toy.outputs(len(ids), lp, lm + 1, lm))
    for keep in (("stop_tokens",), ("phonemes",), ("valid_len",), ("loss_mask",), ("spectrogram_input",), ("spectrogram_target", "valid_len"),
                 ("spectrogram_input", "stop_tokens")):
        out = {k: v for k, v in toy.outputs(len(ids), lp, lm + 1, lm).items() if k in keep}
        _same(toy.launch(ids, lm, out), full, keep)
    # every output has its own row count
    out = toy.outputs(len(ids), lp, 70, 200)
    out["stop_tokens"], out["loss_mask"] = out["stop_tokens"][:, :3].contiguous(), out["loss_mask"][:, :129].contiguous()
    got = toy.launch(ids, lm, out, valid_in=66)
    pads = dict(spectrogram_input=ref.collate([toy.items[i] for i in ids], toy.n_mel, R_in=70, valid_in=66)["spectrogram_input"])
    for key, rows in (("spectrogram_target", 200), ("stop_tokens", 3), ("loss_mask", 129)):
        pads[key] = ref.collate([toy.items[i] for i in ids], toy.n_mel, R=rows)[key]
    _same(got, pads)


# ------------------------------------------------------------------ 5. refusals
def test_bad_arguments_are_refused_before_any_launch(gpu):
    from reformer_tts_amd import _lib, ops
    toy = _Toy(gpu, 8)
    c = toy.corpus
    ids = torch.tensor([5, 1], dtype=torch.int32, device=gpu)
    out = toy.outputs(2, 65, 131, 130)
    base = dict(mel=c.mel.data_ptr(), ld_mel=c.mel.shape[1], fo=c.tables[0].data_ptr(), ph=c.phoneme_ids.data_ptr(), n_ph=c.phoneme_ids.numel(),
                po=c.tables[1].data_ptr(), n_utt=7, ids=ids.data_ptr(), B=2, n_mel=8, lm=130, phonemes=out["phonemes"].data_ptr(), LP=65,
                spec_in=out["spectrogram_input"].data_ptr(), R_in=131, valid_in=131, spec_tgt=out["spectrogram_target"].data_ptr(), R_tgt=130,
                stop=out["stop_tokens"].data_ptr(), R_stop=130, mask=out["loss_mask"].data_ptr(), R_mask=130, valid_len=out["valid_len"].data_ptr(),
                noise_std=0.0, seed=0)
    bad = [(dict(mel=None), "mel is a null"), (dict(fo=None), "frame_offsets is a null"), (dict(ph=None), "phoneme_ids is a null"),
           (dict(po=None), "phoneme_offsets is a null"), (dict(ids=None), "ids is a null"), (dict(B=0), "B must be in 1..65535"),
           (dict(B=65536), "B must be in 1..65535"), (dict(n_mel=0), "n_mel must be in 1..128"), (dict(n_mel=129), "n_mel must be in 1..128"),
           (dict(LP=0), "LP must be positive"), (dict(R_in=0), "R_in must be positive"), (dict(R_tgt=0), "R_target must be positive"),
           (dict(R_stop=-1), "R_stop must be positive"), (dict(R_mask=0), "R_mask must be positive"), (dict(valid_in=132), "valid_in must be in"),
           (dict(valid_in=0), "valid_in must be in"), (dict(n_utt=0), "n_utt must be positive"),
           (dict(phonemes=None, spec_in=None, spec_tgt=None, stop=None, mask=None, valid_len=None), "every output is a null")]
    for change, message in bad:
        with pytest.raises(_lib.RttsError, match=message):
            _lib.call("rtts_tts_collate", *{**base, **change}.values(), torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        ops.tts_collate(c.mel.cpu(), c.tables[0], c.phoneme_ids, c.tables[1], ids, 130, **out)
    with pytest.raises(_lib.RttsError, match="GPU only"):
        ops.tts_collate(c.mel, c.tables[0], c.phoneme_ids, c.tables[1], ids.cpu(), 130, **out)
    with pytest.raises(ValueError, match="loss_mask"):
        ops.tts_collate(c.mel, c.tables[0], c.phoneme_ids, c.tables[1], ids, 130, **{**out, "loss_mask": out["loss_mask"][:, :, :7]})
    torch.cuda.synchronize()
    for k, v in out.items():                                                         # nothing was launched: no word was written
        assert bool(torch.isnan(v).all() if v.is_floating_point() else (v == -1).all()), k
    _lib.call("rtts_tts_collate", *base.values(), torch.cuda.current_stream().cuda_stream)       # and the unchanged call is fine
    torch.cuda.synchronize()
    assert not torch.isnan(out["spectrogram_input"]).any() and int(out["valid_len"]) == 130


# ------------------------------------------------------------------ 6. input noise
@pytest.mark.parametrize("ids", CASES, ids=str)
def test_input_noise(toy, ids):
    lp, lm = toy.shape(ids)
    b, nm, seed = len(ids), toy.n_mel, 0x1234567
    LM = -(-lm // 128) * 128
    clean_ref = toy.launch(ids, lm, toy.outputs(b, lp, lm + 1, lm))
    clean_pad = toy.launch(ids, lm, toy.outputs(b, lp, LM, LM), valid_in=lm)
    _same(toy.launch(ids, lm, toy.outputs(b, lp, lm + 1, lm), noise_std=0.0, seed=seed), clean_ref)         # std 0: the stage is not there
    _same(toy.launch(ids, lm, toy.outputs(b, lp, LM, LM), valid_in=lm, noise_std=-1.0, seed=seed), clean_pad)
    worst = {}
    for std in (0.01, 1.0):
        got_ref = toy.launch(ids, lm, toy.outputs(b, lp, lm + 1, lm), noise_std=std, seed=seed)
        got_pad = toy.launch(ids, lm, toy.outputs(b, lp, LM, LM), valid_in=lm, noise_std=std, seed=seed)
        for got, clean in ((got_ref, clean_ref), (got_pad, clean_pad)):               # everything but the input is untouched
            _same(got, clean, [k for k in clean if k != "spectrogram_input"])
        bound = 1e-5 * std + 2e-6
        for k, u in enumerate(ids):
            n = ref.MEL_LENGTHS[u]
            z = ref.noise64(seed, k, n, nm)
            want = toy.items[u]["spectrogram"].double() + std * z
            x = got_ref["spectrogram_input"][k]
            err = (x[1:1 + n].double() - want).abs().max().item()
            worst[std] = max(worst.get(std, 0.0), err)
            assert not x[0].any() and not x[1 + n:].any()                             # start frame and padding stay zero
            live = min(n, lm - 1)                                                     # the padded layout stops at valid_in = lm
            p = got_pad["spectrogram_input"][k]
            assert torch.equal(p[1:1 + live], x[1:1 + live]) and not p[0].any() and not p[1 + live:].any()
            assert (x[1:1 + n] != clean_ref["spectrogram_input"][k, 1:1 + n]).float().mean() > 0.9
        print(f"\n[input noise, n_mel {nm}, ids {ids}] std {std}: max |out - (mel + std z64)| = {worst[std]:.3e} (bound {bound:.3e})")
        assert worst[std] <= bound, (std, worst[std], bound)
    other = toy.launch(ids, lm, toy.outputs(b, lp, lm + 1, lm), noise_std=1.0, seed=seed + 1)
    assert (other["spectrogram_input"] != got_ref["spectrogram_input"]).float().sum() > 0.9 * sum(ref.MEL_LENGTHS[u] for u in ids) * nm
    if ids == [0, 0, 3]:                                                             # the slot, not the utterance, keys the noise
        assert not torch.equal(got_ref["spectrogram_input"][0], got_ref["spectrogram_input"][1])
    batch = toy.corpus.collate(ids, noise_std=1.0, seed=seed)                         # the corpus's two forms carry the same noise
    frames = toy.corpus.frames(ids, noise_std=1.0, seed=seed)
    torch.cuda.synchronize()
    assert torch.equal(batch["spectrogram"].cpu(), got_ref["spectrogram_input"])
    assert torch.equal(frames["spectrogram_input"].cpu(), got_pad["spectrogram_input"][:, :lm])
    assert torch.equal(frames["spectrogram_target"].cpu(), clean_ref["spectrogram_target"])


# ------------------------------------------------------------------ 7. the other constructors
def test_corpus_from_waveforms_and_from_a_vocoder_corpus(gpu):
    from reformer_tts_amd.dataset import TTSCorpus
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram
    from reformer_tts_amd.squeeze_wave.corpus import VocoderCorpus
    creator = Tacotron2Spectrogram(22050, 1024, 1024, 256, 80).to(gpu)
    g = torch.Generator().manual_seed(3)
    waves = [0.1 * torch.randn(n, generator=g) for n in (3000, 700, 5121)]
    ids = [[3, 1, 2], [7], list(range(1, 40))]
    mel, foff = creator.forward_packed(torch.cat(waves).to(gpu), [w.numel() for w in waves])
    items = [dict(phonemes=torch.tensor(p), spectrogram=mel[:, foff[k]:foff[k + 1]].t().cpu()) for k, p in enumerate(ids)]
    want = TTSCorpus.from_items(items, gpu).collate([2, 0, 1])
    vc = VocoderCorpus.from_waveforms(waves, creator)
    shared = TTSCorpus.from_vocoder_corpus(vc, ids)
    assert shared.mel.data_ptr() == vc.mel.data_ptr() and shared.frame_lengths == [n // 256 + 1 for n in (3000, 700, 5121)]
    for corpus in (shared, TTSCorpus.from_waveforms(waves, ids, creator)):
        got = corpus.collate([2, 0, 1])
        torch.cuda.synchronize()
        _same(got, want)
        assert torch.equal(corpus.item(1)["phonemes"].cpu(), torch.tensor([7])) and corpus.item(1)["spectrogram"].shape == (3, 80)
    train, val, test = shared.split((0.34, 0.33, 0.33), seed=1)
    assert sorted(train + val + test) == [0, 1, 2] and (len(train), len(val), len(test)) == (3, 0, 0)
    with pytest.raises(ValueError, match="phoneme id lists"):
        TTSCorpus.from_vocoder_corpus(vc, ids[:2])
