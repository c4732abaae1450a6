"""GPU: a track of 16-bit samples (AudioTrack.from_pcm16 / from_wav; hmm_audio_pcm16_gather_clips, hmm_audio_pcm16_window_sums,
hmm_segment_walk_pcm16) against its oracle, the float64 track AudioTrack(x.astype(np.float64).reshape(-1, 1) / 32768.0, rate) --
what the reference's sf.read makes of the same WAV.  Bit equality everywhere: clips at 16 kHz (head, body and tail of the 16-byte
path) and at four other rates, mel spectrograms, window sums and levels at every length where the float64 kernel changes its
summation tree, the segments of both walks, the embeddings of the audio tower and the bytes of a checkpoint."""
import warnings

import numpy as np
import pytest
import torch

import checkpoint_cases as K

pytestmark = pytest.mark.gpu

SR = 16000
N16 = 80007
SPANS16 = [(0, 40000), (1, 33001), (7, 7 + 11200), (8, 48000), (9, N16)]        # 0.7 s at sample 7; the last one ends with the track
LENGTHS = (0, 1, 7, 8, 9, 127, 128, 129, 8000, 8192, 8193, 1 << 22)
STARTS = (0, 1, 3, 8)


def _pcm(n, seed, scale=32768):
    x = np.random.default_rng(seed).integers(-scale, scale, size=n, dtype=np.int64).astype(np.int16)
    return x


def _pair(x, rate):
    """-> (the PCM track, its oracle)"""
    from hippomm_amd.audio_track import AudioTrack
    return AudioTrack.from_pcm16(x, rate), AudioTrack(x.astype(np.float64).reshape(-1, 1) / 32768.0, rate)


def _bits(t):
    return t.view(torch.int32).cpu()


def _same_clips(got, want):
    assert [(p, c.shape) for p, c in got] == [(p, c.shape) for p, c in want]
    for (positions, g), (_, w) in zip(got, want):
        assert g.dtype == torch.float32 and torch.equal(_bits(g), _bits(w)), positions


@pytest.fixture(scope="module")
def tracks16():
    x = _pcm(N16, 1)
    x[5], x[12345], x[N16 - 1], x[8], x[40000 - 1] = -32768, 32767, -32768, 32767, -32768
    pcm, f64 = _pair(x, SR)
    return x, pcm, f64, f64.segment_clips(SPANS16), f64.melspec(SPANS16)


# ---- attributes ------------------------------------------------------------------------------------------------------------------
def test_a_pcm_track_says_what_it_is(tracks16):
    from hippomm_amd.audio_track import AudioTrack
    x, pcm, f64, _, _ = tracks16
    assert pcm.pcm is True and f64.pcm is False
    assert pcm.samples.dtype == torch.int16 and pcm.samples.shape == (N16,) and np.array_equal(pcm.samples.cpu().numpy(), x)
    assert (pcm.n_samples, pcm.source_dtype, pcm.source_shape, pcm.dtype_code) == (N16, np.float64, (N16, 1), 1)
    assert (f64.n_samples, f64.source_dtype, f64.source_shape, f64.dtype_code) == (N16, np.float64, (N16, 1), 1)
    got = pcm.as_float64(5, 1000)
    assert got.dtype == np.float64 and got.shape == (995, 1) and np.array_equal(got, x[5:1000].astype(np.float64).reshape(-1, 1) / 32768.0)
    assert np.array_equal(pcm.as_float64(), x.astype(np.float64).reshape(-1, 1) / 32768.0)
    assert AudioTrack.from_pcm16(x.reshape(-1, 1), SR).samples.shape == (N16,)
    for wrong in (x.astype(np.int32), x.astype(np.float32), x.astype(np.uint16)):
        with pytest.raises(TypeError, match="int16"):
            AudioTrack.from_pcm16(wrong, SR)
    with pytest.raises(TypeError):
        f64.as_float64()
    peaks = pcm.span_peaks(np.array([(0, 5), (0, 6), (12345, 12346), (100, 100)], dtype=np.int64))
    want = [np.abs(x[0:5].astype(np.float32) / 32768).max(), 1.0, 32767 / 32768, 0.0]
    assert peaks.dtype == torch.float32 and peaks.cpu().tolist() == [float(np.float32(v)) for v in want]


def test_stereo_samples_take_the_float_constructor():
    from hippomm_amd.audio_track import AudioTrack
    s = _pcm(2 * 4001, 2).reshape(-1, 2)
    got, want = AudioTrack.from_pcm16(s, SR), AudioTrack(s.astype(np.float64) / 32768.0, SR)
    assert got.pcm is False and got.samples.dtype == torch.float64 and torch.equal(got.samples, want.samples)


def test_from_wav_holds_the_files_samples(tmp_path):
    from scipy.io import wavfile
    from hippomm_amd.audio_track import AudioTrack
    x = _pcm(56005, 3)
    x[0], x[-1] = -32768, 32767
    wavfile.write(tmp_path / "temp_audio.wav", 22050, x)
    track = AudioTrack.from_wav(tmp_path / "temp_audio.wav")
    assert track.pcm and track.sample_rate == 22050 and track.n_samples == 56005
    assert track.samples.dtype == torch.int16 and np.array_equal(track.samples.cpu().numpy(), x)


# ---- clips -----------------------------------------------------------------------------------------------------------------------
def test_16k_clips_and_melspec_are_the_float64_tracks_bits(tracks16):
    x, pcm, f64, want_clips, want_mel = tracks16
    got = pcm.segment_clips(SPANS16)
    assert sorted(c.shape[1] for _, c in got) == [11200, 32000]
    _same_clips(got, want_clips)
    f = (x.astype(np.float32) / np.float32(32768))                          # and they are the samples themselves
    (positions, clips), = [g for g in got if g[1].shape[1] == 11200]
    assert positions == [2] and np.array_equal(clips[0].cpu().numpy(), f[7:7 + 11200])
    mel = pcm.melspec(SPANS16)
    assert mel.shape == (len(SPANS16), 3, 1, 128, 204) and torch.equal(_bits(mel), _bits(want_mel))


def test_a_span_has_the_same_clip_bits_alone_among_others_and_again(tracks16):
    x, pcm, f64, want_clips, _ = tracks16
    together = {p: c for positions, c in pcm.segment_clips(SPANS16) for p, c in zip(positions, c.view(len(positions), 3, -1))}
    for s, span in enumerate(SPANS16):
        (positions, alone), = pcm.segment_clips([span])
        assert positions == [0] and torch.equal(_bits(alone.view(3, -1)), _bits(together[s])), span
    _same_clips(pcm.segment_clips(SPANS16), want_clips)                     # a second call


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000])
def test_resampled_clips_are_the_float64_tracks_bits(rate):
    n = 3 * rate
    x = _pcm(n, rate)
    x[0], x[1], x[n - 1] = -32768, 32767, -32768
    pcm, f64 = _pair(x, rate)
    spans = [(0, n), (1, n), (7, 7 + int(0.7 * rate)), (n - 2 * rate - 3, n)]
    want = f64.segment_clips(spans)
    _same_clips(pcm.segment_clips(spans), want)
    (positions, alone), = pcm.segment_clips([spans[3]])
    both = {p: c for ps, c in want for p, c in zip(ps, c.view(len(ps), 3, -1))}
    assert torch.equal(_bits(alone.view(3, -1)), _bits(both[3]))


# ---- sums and levels -------------------------------------------------------------------------------------------------------------
def test_window_sums_are_exact_and_the_float64_tracks_bits():
    from hippomm_amd._lib import HippoMMHipError
    n = (1 << 22) + 16
    x = _pcm(n, 5)
    x[3], x[4000] = -32768, 32767
    pcm, f64 = _pair(x, SR)
    table = np.array([(a, m) for m in LENGTHS for a in STARTS], dtype=np.int64)
    got = pcm.window_sums(table)
    sq = np.concatenate([[0], np.cumsum(np.square(x.astype(np.int64)))])
    exact = np.array([int(sq[a + m] - sq[a]) * 2.0 ** -30 for a, m in table.tolist()])
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), exact.view(np.uint64))
    assert np.array_equal(got.view(np.uint64), f64.window_sums(table).view(np.uint64))
    assert np.array_equal(pcm.window_sums(table[::-1].copy()).view(np.uint64), got[::-1].view(np.uint64))    # nor on the batch
    with pytest.raises(HippoMMHipError, match="2\\^22"):                    # inside the track, but no longer exact: refused
        pcm.window_sums(np.array([(0, 8), (2, (1 << 22) + 1)], dtype=np.int64))
    assert pcm.window_sums(np.empty((0, 2), dtype=np.int64)).shape == (0,)


def test_a_window_of_2_to_the_22_samples_at_full_scale_sums_to_2_to_the_22():
    from hippomm_amd.audio_track import AudioTrack
    pcm = AudioTrack.from_pcm16(np.full((1 << 22) + 1, -32768, dtype=np.int16), SR)
    got = pcm.window_sums(np.array([(0, 1 << 22), (1, 1 << 22), (1, 9)], dtype=np.int64))
    assert got.tolist() == [2.0 ** 22, 2.0 ** 22, 9.0]


def test_window_levels_are_the_host_expression_in_value_and_type():
    from hippomm_amd.segmentation import audio_level
    n = 20011
    x = _pcm(n, 6, scale=3000)
    x[4000:9000] = 0                                                        # silence: the int -100
    pcm, f64 = _pair(x, SR)
    f = x.astype(np.float64).reshape(-1, 1) / 32768.0
    starts = [0, 1, 3, 8, 4000, 4100, 8999, n - 8000, n - 5, n, n + 7]      # the last two are empty, the two before run off the end
    for window in (8000, 129, 1):
        got = pcm.window_level_values(starts, window)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = [audio_level(f[lo:lo + window], SR) for lo in starts]
        assert [type(v) for v in got] == [type(v) for v in want], window
        assert [repr(v) for v in got] == [repr(v) for v in want], window
        assert -100 in got and got == f64.window_level_values(starts, window)
        levels = pcm.window_levels(starts, window)
        assert levels.dtype == np.float64 and np.array_equal(levels, np.asarray(want, dtype=np.float64))


# ---- segmentation ----------------------------------------------------------------------------------------------------------------
def test_both_walks_give_the_float64_tracks_segments():
    from hippomm_amd.segmentation import segment_sequence
    rate, n = 1000, 60 * 1000
    x = _pcm(n, 7, scale=3000)
    for a, b in ((7400, 8100), (21250, 22900), (40010, 40600), (55000, 55499)):
        x[a:b] = 0
    x[30000:30700] = _pcm(700, 8, scale=600)                                # about -39.5 dB: quiet, just not silent at -40
    pcm, f64 = _pair(x, rate)
    f = x.astype(np.float64).reshape(-1, 1) / 32768.0
    want = [(s.start_time, s.end_time) for s in segment_sequence(None, None, f, rate)]
    assert len(want) > 4
    for walk in ("host", "device"):
        for track in (f64, pcm):
            stats = {}
            got = segment_sequence(None, None, None, rate, audio_track=track, walk=walk, stats=stats)
            assert stats["route"] == walk, stats
            assert [(s.start_time, s.end_time) for s in got] == want, (walk, track.pcm)
    got = segment_sequence(None, None, f, rate, audio_track=pcm, walk="device")
    assert all(np.shares_memory(s.audio_data, f) for s in got) and [(s.start_time, s.end_time) for s in got] == want


# ---- the tower and the checkpoint --------------------------------------------------------------------------------------------------
def test_extract_audio_segments_gives_the_float64_tracks_embeddings(tracks16):
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    x, pcm, f64, _, _ = tracks16
    model = ImageBind(state_dict=synthetic_state_dict(("audio",), depth={"audio": 2}), towers=("audio",), depth={"audio": 2})
    spans = [SPANS16[1], SPANS16[2], SPANS16[4]]
    got = model.extract_audio_segments(pcm, SR, spans)
    assert got.shape == (3, 1024) and got.dtype == torch.float32
    assert torch.equal(_bits(got), _bits(model.extract_audio_segments(f64, SR, spans)))


def test_a_checkpoint_has_the_same_bytes_from_a_pcm_track(tracks16):
    from hippomm_amd import checkpoint as ck
    x, pcm, f64, _, _ = tracks16
    span = (9, 9 + SR // 4)                                                 # 0.25 s
    recipe = dict(K.RECIPE, frames=[2], spans=[list(span)], times=[[0.0, 0.25]], transcriptions=["a quarter of a second"])
    memories = K.recipe_memories(recipe, track=pcm.as_float64())
    assert memories[0].segment_info.audio_data.shape == (SR // 4, 1)
    host = ck.checkpoint_bytes("v", memories, 12.5, matrices="host")
    for track in (pcm, f64):
        stats = {}
        got = ck.checkpoint_bytes("v", memories, 12.5, matrices="device", audio_track=track, audio_spans=[span], stats=stats)
        assert got == host, track.pcm
        assert (stats["waveform_resident"], stats["waveform_upload"], stats["waveform_host"]) == (1, 0, 0), (track.pcm, stats)
