"""``rtts_sw_draw_segments`` and the corpus trainer on the GPU.

Kernel level: a synthetic corpus that owes nothing to the mel kernel (tests/sw_corpus_ref.py: audio = arange, mel = m * 1e5 +
column, sentinel columns behind the frames, outputs prefilled with NaN) against ``vocoder_segment`` bit for bit -- every
utterance and legal hop through ``picks_in``, f32 and int16 sources, drawn batches inside a replayed graph against the
reference draw, a wider mel row stride, strangers in ``order`` / ``picks_in``, and every refusal.

Trainer level: ``VocoderTrainer.capture_corpus`` against the existing ``capture`` graph fed the same crops assembled on the host
from the recorded picks: identical rows into an identical deterministic launch list, so everything is bit-equal."""
import wave

import numpy as np
import pytest
import torch

import sw_corpus_ref as ref
import sw_train_ref as train64
from test_sw_train_graph_hip import _assert_same_state, _build, _state

pytestmark = pytest.mark.gpu

B = 7


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class _Toy:
    """The toy corpus on the device (``fmt`` 0: f32, 1: int16) with the host copies the expectations are made from."""

    def __init__(self, gpu, n_mel, fmt):
        audio, self.so, self.mel, self.fo = ref.toy_corpus(n_mel)
        pcm = audio.to(torch.int16)
        self.audio = pcm.float() / 32768 if fmt else audio                     # what the kernel is to deliver
        self.d_audio = (pcm if fmt else audio).to(gpu)
        self.d_mel = self.mel.to(gpu)
        self.d_so, self.d_fo = torch.tensor(self.so, device=gpu), torch.tensor(self.fo, device=gpu)
        self.n_mel, self.gpu = n_mel, gpu

    def outputs(self, batch, ld_rows=None):
        nan = float("nan")
        return (torch.full((batch * ref.S // ref.C, ref.C), nan, device=self.gpu),
                torch.full((batch * ref.SEG_FRAMES, ld_rows or self.n_mel), nan, device=self.gpu),
                torch.full((batch, 2), -99, dtype=torch.int32, device=self.gpu))

    def draw(self, batch, out, picks=None, order=None, state=None, seed=0):
        from reformer_tts_amd import ops
        ops.sw_draw_segments(self.d_audio, self.d_so, self.d_mel, self.d_fo, order, state, seed, picks, batch, ref.SEG_FRAMES, ref.HOP, ref.C, *out)

    def expect(self, picks):
        """-> (audio rows, mel rows) of ``picks`` from ``vocoder_segment``; a (-1, 0) pick is an all-zero segment."""
        a, m = [], []
        for u, h in picks:
            if u < 0:
                wa, wm = torch.zeros(ref.S), torch.zeros(ref.SEG_FRAMES, self.n_mel)
            else:
                wa, wm = ref.segment_rows(self.audio[self.so[u]:self.so[u + 1]], self.mel[:, self.fo[u]:self.fo[u + 1]], h)
            a.append(wa)
            m.append(wm)
        return torch.stack(a).view(-1, ref.C), torch.cat(m)

    def check(self, out, picks):
        audio_rows, mel_rows, picks_out = (t.cpu() for t in out)
        wa, wm = self.expect(picks)
        assert picks_out.tolist() == [list(p) for p in picks]
        assert torch.equal(audio_rows, wa)
        assert torch.equal(mel_rows[:, :self.n_mel], wm)
        assert not (mel_rows == ref.SENTINEL).any()


# ------------------------------------------------------------------ 1. every utterance, every legal hop
@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "int16"])
@pytest.mark.parametrize("n_mel", [80, 8])
def test_every_utterance_and_hop_is_vocoder_segment(gpu, n_mel, fmt):
    toy = _Toy(gpu, n_mel, fmt)
    picks = ref.all_picks()
    for lo in range(0, len(picks), B):
        group = (picks[lo:lo + B] + picks[:B])[:B]
        out = toy.outputs(B)
        toy.draw(B, out, picks=torch.tensor(group, dtype=torch.int32, device=gpu))
        toy.check(out, group)
    # the restatement agrees with vocoder_segment on the same picks (tests/test_sw_corpus_cpu.py), here once more end to end
    a, m = ref.gather(toy.audio, toy.so, toy.mel, toy.fo, picks)
    wa, wm = toy.expect(picks)
    assert torch.equal(a.view(-1, ref.C), wa) and torch.equal(m, wm)


# ------------------------------------------------------------------ 2. drawn inside a replayed graph
@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "int16"])
def test_drawn_batches_in_a_replayed_graph(gpu, fmt):
    from reformer_tts_amd._graphs import warm_capture
    toy = _Toy(gpu, 80, fmt)
    batch, seed, order = 4, 0x9E3779B9, [2, 5, 0, 3, 4, 1]
    d_order = torch.tensor(order, dtype=torch.int32, device=gpu)
    state = torch.tensor([0, 17], dtype=torch.int64, device=gpu)
    out = toy.outputs(batch)

    def step():
        toy.draw(batch, out, order=d_order, state=state, seed=seed)
        state[0:1].add_(batch)

    graph, _ = warm_capture(step)
    state.copy_(torch.tensor([0, 17]))                                          # the warm-up drew once
    seen = []
    for cursor, epoch_seed in ((0, 17), (4, 17), (8, 18)):
        state[1:2].fill_(epoch_seed)                                            # on the device, between replays: no recapture
        for t in out[:2]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = ref.draw_picks(cursor, epoch_seed, seed, order, ref.LENGTHS, batch)
        toy.check(out, want)
        seen.append(want)
        assert int(state[0]) == cursor + batch
    assert [u for u, _ in seen[1]] == [4, 1, 2, 5]                              # i = 6, 7 wrapped to order[0], order[1]
    assert [u for u, _ in seen[2]] == [0, 3, 4, 1]
    # the third batch holds no utterance with a choice of hops; cursor 0 again, under both epoch seeds, holds the two long ones
    both = []
    for epoch_seed in (17, 18):
        state.copy_(torch.tensor([0, epoch_seed]))
        graph.replay()
        torch.cuda.synchronize()
        want = ref.draw_picks(0, epoch_seed, seed, order, ref.LENGTHS, batch)
        toy.check(out, want)
        both.append(want)
    assert [u for u, _ in both[0]] == [u for u, _ in both[1]] == [2, 5, 0, 3]
    assert both[0] != both[1]
    assert seen[0] == both[0]


# ------------------------------------------------------------------ 3. a wider output row
def test_wider_mel_rows_keep_their_spare_columns(gpu):
    toy = _Toy(gpu, 80, 0)
    picks = ref.all_picks()[3:3 + B]
    out = toy.outputs(B, ld_rows=83)
    toy.draw(B, out, picks=torch.tensor(picks, dtype=torch.int32, device=gpu))
    toy.check(out, picks)
    assert torch.isnan(out[1][:, 80:]).all()
    # a strided view of a wider buffer: the same through the row stride alone
    wide = torch.full((B * ref.SEG_FRAMES, 96), float("nan"), device=gpu)
    out2 = (toy.outputs(B)[0], wide[:, :80], out[2])
    toy.draw(B, out2, picks=torch.tensor(picks, dtype=torch.int32, device=gpu))
    toy.check(out2, picks)
    assert torch.isnan(wide[:, 80:]).all()


# ------------------------------------------------------------------ 3b. the other paths of the kernel
@pytest.mark.parametrize("seg_frames,hop,c,n_mel,fmt", [(3, 5, 5, 3, 0), (3, 5, 1, 3, 1), (70, 64, 128, 5, 0), (70, 64, 128, 128, 1)])
def test_odd_segments_and_more_than_one_tile(gpu, seg_frames, hop, c, n_mel, fmt):
    """S = 15: every second slot starts off the 16-byte grid (the element path) and S % 4 != 0 (a tail behind the vectors);
    seg_frames 70, S = 4480: two mel tiles and two audio tiles, the second of each partial; n_mel 128: the widest tile."""
    from reformer_tts_amd import ops
    from reformer_tts_amd.dataset.utils import vocoder_segment
    s = seg_frames * hop
    g = torch.Generator().manual_seed(s)
    lengths = [s, 2 * s + 3, s - 1, s // 2 + 1, s + 2 * hop + 1]
    pcm = [torch.randint(-32768, 32767, (n,), generator=g).to(torch.int16) for n in lengths]
    audios = [p.float() / 32768 for p in pcm] if fmt else [torch.randn(n, generator=g) for n in lengths]
    mels = [torch.randn(n_mel, n // hop + 1, generator=g) for n in lengths]
    so, fo = [0], [0]
    for n, m in zip(lengths, mels):
        so.append(so[-1] + n)
        fo.append(fo[-1] + m.shape[1])
    picks = [(u, h) for u, n in enumerate(lengths) for h in range(max((n - s) // hop, 0) + 1)]
    nb = len(picks)
    out = (torch.full((nb * s // c, c), float("nan"), device=gpu), torch.full((nb * seg_frames, n_mel), float("nan"), device=gpu),
           torch.full((nb, 2), -99, dtype=torch.int32, device=gpu))
    ops.sw_draw_segments(torch.cat(pcm if fmt else audios).to(gpu), torch.tensor(so, device=gpu), torch.cat(mels, dim=1).to(gpu),
                         torch.tensor(fo, device=gpu), None, None, 0, torch.tensor(picks, dtype=torch.int32, device=gpu), nb, seg_frames, hop, c, *out)
    want = [vocoder_segment(audios[u], mels[u], s, hop, random_hop=h) for u, h in picks]
    assert out[2].cpu().tolist() == [list(p) for p in picks]
    assert torch.equal(out[0].cpu().view(nb, s), torch.stack([a for a, _ in want]))
    assert torch.equal(out[1].cpu().view(nb, seg_frames, n_mel), torch.stack([m.t() for _, m in want]))


# ------------------------------------------------------------------ 4. strangers
def test_unknown_utterances_give_zero_segments(gpu):
    toy = _Toy(gpu, 8, 0)
    picks = [(2, 3), (6, 0), (5, 4), (-1, 2), (0, 0), (1 << 30, 1), (4, 0)]
    out = toy.outputs(B)
    toy.draw(B, out, picks=torch.tensor(picks, dtype=torch.int32, device=gpu))
    toy.check(out, [(u, h) if 0 <= u < 6 else (-1, 0) for u, h in picks])
    order = [3, 6, 2, -4, 5, 1, 0]
    out = toy.outputs(B)
    state = torch.tensor([0, 1], dtype=torch.int64, device=gpu)
    toy.draw(B, out, order=torch.tensor(order, dtype=torch.int32, device=gpu), state=state, seed=9)
    want = ref.draw_picks(0, 1, 9, order, ref.LENGTHS, B)
    assert [u for u, _ in want] == [3, -1, 2, -1, 5, 1, 0]
    toy.check(out, want)
    assert state.tolist() == [0, 1]                                             # the kernel only reads it


# ------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_argument_and_launch_nothing(gpu):
    from reformer_tts_amd import _lib
    toy = _Toy(gpu, 80, 0)
    out = toy.outputs(B)
    order = torch.arange(6, dtype=torch.int32, device=gpu)
    state = torch.zeros(2, dtype=torch.int64, device=gpu)
    picks = torch.zeros(B, 2, dtype=torch.int32, device=gpu)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(audio=toy.d_audio.data_ptr(), in_format=0, n_audio=toy.d_audio.numel(), sample_offsets=toy.d_so.data_ptr(),
                mel=toy.d_mel.data_ptr(), ld_mel=toy.d_mel.stride(0), frame_offsets=toy.d_fo.data_ptr(), n_utt=6, order=order.data_ptr(),
                n_order=6, state=state.data_ptr(), seed=1, picks_in=None, B=B, seg_frames=ref.SEG_FRAMES, hop=ref.HOP,
                C=ref.C, n_mel=80, audio_rows=out[0].data_ptr(), mel_rows=out[1].data_ptr(), ld_mel_rows=80, picks_out=out[2].data_ptr())

    def refused(match, **change):
        args = dict(good, **change)
        with pytest.raises(_lib.RttsError, match=match):
            _lib.call("rtts_sw_draw_segments", *args.values(), stream)

    for name in ("audio", "sample_offsets", "mel", "frame_offsets", "audio_rows", "mel_rows", "picks_out", "order", "state"):
        refused(rf"rtts_sw_draw_segments: {name} is a null pointer", **{name: None})
    for name in ("B", "seg_frames", "hop", "C", "n_mel"):
        refused(rf"rtts_sw_draw_segments: {name} must be", **{name: 0})
        refused(rf"rtts_sw_draw_segments: {name} must be", **{name: -3})
    refused(r"n_mel must be in 1\.\.128 \(got 129\)", n_mel=129, ld_mel_rows=129)
    refused(r"seg_frames \* hop = 1024 is not a multiple of C = 100", C=100)
    refused(r"in_format must be 0 \(f32\) or 1 \(int16 mono\), got 2", in_format=2)
    refused(r"in_format must be", in_format=-1)
    refused(r"n_order must be positive", n_order=0)
    refused(r"ld_mel_rows = 79 is smaller than n_mel = 80", ld_mel_rows=79)
    torch.cuda.synchronize()
    assert torch.isnan(out[0]).all() and torch.isnan(out[1]).all() and (out[2] == -99).all()
    # with picks_in the draw's tables are not needed: order, state and n_order may be empty
    _lib.call("rtts_sw_draw_segments", *dict(good, order=None, state=None, n_order=0, picks_in=picks.data_ptr()).values(), stream)
    toy.check(out, [(0, 0)] * B)
    # the tensor wrapper refuses host tensors by name, before the library is reached
    with pytest.raises(_lib.RttsError, match="GPU only: mel must be"):
        from reformer_tts_amd import ops
        ops.sw_draw_segments(toy.d_audio, toy.d_so, toy.mel, toy.d_fo, order, state, 0, None, B, ref.SEG_FRAMES, ref.HOP, ref.C, *toy.outputs(B))


# ------------------------------------------------------------------ 6. the corpus trainer
def _random_corpus(golden_dir, case, gpu):
    """A corpus of six random utterances around the case's segment length -> (corpus, host audio list, host mel list, cfg)."""
    from reformer_tts_amd.squeeze_wave.corpus import VocoderCorpus
    cfg, _, mel, _ = train64.load_train_case(golden_dir, case)
    batch, n_mel, mel_len = mel.shape
    s = 256 * mel_len
    g = torch.Generator().manual_seed(mel_len)
    lengths = [s, s + 3 * 256 + 5, s - 1, 2 * s, s + 700, s // 2 + 3]
    audios = [0.1 * torch.randn(n, generator=g) for n in lengths]
    mels = [torch.randn(n_mel, n // 256 + 1, generator=g) for n in lengths]
    foff = [0]
    for m in mels:
        foff.append(foff[-1] + m.shape[1])
    corpus = VocoderCorpus.from_packed(torch.cat(audios).to(gpu), lengths, torch.cat(mels, dim=1).to(gpu), foff, 256)
    return corpus, audios, mels, cfg, batch, mel_len


def _host_batch(audios, mels, picks, s, gpu):
    """What the parent's training loop assembles on the host: ``vocoder_segment`` per utterance, stacked."""
    from reformer_tts_amd.dataset.utils import vocoder_segment
    pairs = [vocoder_segment(audios[u], mels[u], s, 256, random_hop=h) for u, h in picks]
    return {"spectrogram": torch.stack([m for _, m in pairs]).to(gpu), "audio": torch.stack([a for a, _ in pairs]).to(gpu)}


def _corpus_against_host_batches(golden_dir, case, gpu, n_steps):
    from reformer_tts_amd.squeeze_wave.corpus import SegmentSampler
    from reformer_tts_amd.squeeze_wave.training import VocoderTrainer
    corpus, audios, mels, cfg, batch, mel_len = _random_corpus(golden_dir, case, gpu)
    am, _, _ = _build(golden_dir, case, gpu)
    bm, _, _ = _build(golden_dir, case, gpu)
    at, bt = VocoderTrainer(am, logdet="device"), VocoderTrainer(bm, logdet="device")
    sampler = SegmentSampler(corpus, batch, 256 * mel_len, seed=5, n_audio_channels=cfg["n_audio_channels"])
    sampler.start_epoch(0)
    order = sampler.order.cpu().tolist()
    run_a = at.capture_corpus(sampler)
    assert sampler.state.tolist() == [0, 0]                                     # the warm-up's draw was undone
    run_b = bt.capture(batch, mel_len)
    _assert_same_state(_state(am, at), _state(bm, bt))                          # ... and so was its step, as capture undoes its own
    losses_a, losses_b, picks = [], [], []
    for _ in range(n_steps):
        losses_a.append(float(run_a()))
        picks.append([tuple(p) for p in run_a.picks.cpu().tolist()])
    for p in picks:
        losses_b.append(float(run_b(_host_batch(audios, mels, p, 256 * mel_len, gpu))))
    torch.cuda.synchronize()
    print(case, "picks", picks, "losses", losses_a, losses_b)
    lengths = [a.numel() for a in audios]
    assert picks == [ref.draw_picks(k * batch, 0, 5, order, lengths, batch, 256 * mel_len, 256) for k in range(n_steps)]
    assert all(l == l for l in losses_a) and losses_a == losses_b
    _assert_same_state(_state(am, at), _state(bm, bt))
    tracked = [int(v) for k, v in am.state_dict().items() if k.endswith("num_batches_tracked")]
    assert tracked and all(t == n_steps for t in tracked)
    assert sampler.state.tolist() == [n_steps * batch, 0]
    # batch_dict shows the last draw in the reference's batch format
    last = _host_batch(audios, mels, picks[-1], 256 * mel_len, gpu)
    got = sampler.batch_dict()
    assert torch.equal(got["spectrogram"], last["spectrogram"]) and torch.equal(got["audio"], last["audio"])
    return at, sampler, run_a


def test_capture_corpus_is_capture_on_the_same_crops_small(golden_dir, gpu):
    """``small``: three replays that draw all six utterances (cropped, exact, padded) against the ``capture`` graph fed the same
    crops from the host: losses, parameters, BatchNorm buffers and Adam state bit-equal."""
    _corpus_against_host_batches(golden_dir, "small", gpu, 3)


def test_capture_corpus_is_capture_on_the_same_crops_full(golden_dir, gpu):
    """``full/3x10``, the MFMA path with its 128-row buffers: one step."""
    _corpus_against_host_batches(golden_dir, "full/3x10", gpu, 1)


def test_fit_corpus_epochs(golden_dir, gpu):
    """Two epochs over a 5-utterance subset at batch 2: two steps each, no utterance twice within an epoch, the remainder dropped,
    another order in the second epoch."""
    from reformer_tts_amd.squeeze_wave.corpus import SegmentSampler
    from reformer_tts_amd.squeeze_wave.training import VocoderTrainer
    corpus, _, _, cfg, batch, mel_len = _random_corpus(golden_dir, "small", gpu)
    model, _, _ = _build(golden_dir, "small", gpu)
    trainer = VocoderTrainer(model, logdet="device")
    subset = [0, 1, 2, 4, 5]
    sampler = SegmentSampler(corpus, batch, 256 * mel_len, indices=subset, seed=3, n_audio_channels=cfg["n_audio_channels"])
    assert batch == 2 and sampler.steps_per_epoch == 2
    run = trainer.capture_corpus(sampler)
    seen, orders = [], []

    def spy():
        if not seen or len(seen) % sampler.steps_per_epoch == 0:
            orders.append(sampler.order.cpu().tolist())
        loss = run()
        seen.append([u for u, _ in run.picks.cpu().tolist()])
        return loss
    spy.sampler = sampler
    losses = trainer.fit_corpus(sampler, 2, run=spy)
    assert len(losses) == 4 and all(l == l for l in losses) and len(orders) == 2
    epochs = [seen[0] + seen[1], seen[2] + seen[3]]
    for used, order in zip(epochs, orders):
        assert sorted(order) == subset
        assert used == order[:4]                                                 # four distinct utterances; order[4] is dropped
    assert orders[0] != orders[1] and epochs[0] != epochs[1]
    assert sampler.state.tolist() == [4, 1] and sampler.epoch == 1
    tracked = [int(v) for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")]
    assert tracked and all(t == 4 for t in tracked)
    with pytest.raises(ValueError, match="not captured from this sampler"):
        trainer.fit_corpus(SegmentSampler(corpus, batch, 256 * mel_len, n_audio_channels=cfg["n_audio_channels"]), 1, run=run)


# ------------------------------------------------------------------ 7. building a corpus
def _write_pcm(path, pcm, channels, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())


def test_corpus_from_waveforms_and_from_directory(gpu, tmp_path):
    """``from_directory`` holds what ``preprocess_directory`` writes, bit for bit, and the audio it was made from; ``pcm16`` keeps the
    16-bit samples and mels of exactly those; a sampler over the result draws ``vocoder_segment`` of the stored pair."""
    from reformer_tts_amd.dataset.audio import Tacotron2Spectrogram, preprocess_directory
    from reformer_tts_amd.dataset.utils import vocoder_segment
    from reformer_tts_amd.squeeze_wave.corpus import SegmentSampler, VocoderCorpus
    creator = Tacotron2Spectrogram(22050, 1024, 1024, 256, 80).to(gpu)
    audio_dir, mel_dir, mono_dir = (tmp_path / d for d in ("wav", "mel", "mono"))
    audio_dir.mkdir()
    mono_dir.mkdir()
    rs = np.random.RandomState(0)
    files = {"a48.wav": (48000, 2, 24000), "b22.wav": (22050, 1, 5000), "c22.wav": (22050, 1, 9000)}
    pcm = {}
    for name, (rate, channels, n) in files.items():
        pcm[name] = rs.randint(-20000, 20000, (n, channels)).astype(np.int16)
        _write_pcm(audio_dir / name, pcm[name], channels, rate)
        if rate == 22050:
            _write_pcm(mono_dir / name, pcm[name], channels, rate)
    preprocess_directory(audio_dir, mel_dir, creator, resample=True)
    corpus = VocoderCorpus.from_directory(audio_dir, creator, resample=True)
    assert sorted(corpus.names) == sorted(files) and len(corpus) == 3 and corpus.audio.dtype == torch.float32
    for u, name in enumerate(corpus.names):
        audio_u, mel_u = corpus.utterance(u)
        assert torch.equal(mel_u.cpu(), torch.load(mel_dir / (name[:-4] + ".pt"))[0]), name
        assert mel_u.shape[1] == audio_u.numel() // 256 + 1
        if files[name][0] == 22050:
            assert torch.equal(audio_u.cpu(), torch.from_numpy(pcm[name][:, 0].astype(np.float32)) / 32768.0)
        else:
            assert audio_u.numel() == 24000 * 22050 // 48000
    with pytest.raises(ValueError):
        VocoderCorpus.from_directory(audio_dir, creator)                         # another rate, stereo: only with resample=True
    # 16-bit storage: the files' own samples, the same mels
    plain = VocoderCorpus.from_directory(mono_dir, creator)
    packed = VocoderCorpus.from_directory(mono_dir, creator, pcm16=True)
    assert packed.audio.dtype == torch.int16 and plain.names == packed.names == ["b22.wav", "c22.wav"]
    assert torch.equal(packed.audio.cpu(), torch.from_numpy(np.concatenate([pcm[n][:, 0] for n in packed.names])))
    assert torch.equal(packed.mel, plain.mel) and packed.frame_offsets == plain.frame_offsets
    # from_waveforms: the same corpus from tensors; f32 waveforms rounded to 16 bits keep audio and mel a pair
    waves = [plain.utterance(u)[0] for u in range(2)]
    again = VocoderCorpus.from_waveforms(waves, creator)
    assert torch.equal(again.audio, plain.audio) and torch.equal(again.mel, plain.mel)
    noisy = [w + 1e-6 for w in waves]
    rounded = VocoderCorpus.from_waveforms(noisy, creator, pcm16=True)
    assert torch.equal(rounded.audio, packed.audio) and torch.equal(rounded.mel, packed.mel)
    # and a draw from it is the reference's crop of the stored pair, short utterance (5000 < 8192) padded
    sampler = SegmentSampler(packed, 2, 8192, seed=1)
    sampler.start_epoch(0)
    sampler.draw()
    torch.cuda.synchronize()
    got = sampler.batch_dict()
    for b, (u, h) in enumerate(sampler.picks.cpu().tolist()):
        a, m = (t.cpu() for t in packed.utterance(u))
        wa, wm = vocoder_segment(a, m, 8192, 256, random_hop=h)
        assert torch.equal(got["audio"][b].cpu(), wa) and torch.equal(got["spectrogram"][b].cpu(), wm)
