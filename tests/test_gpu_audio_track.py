"""GPU: the audio track on the device (hippomm_amd/audio_track.py, csrc/audio_track.hip) against the route it stands for -- the
reference's per-segment wav files through load_and_transform_audio_data_device / extract_features.

16 kHz: the clips, the mel spectrograms and the embeddings of a batch are the file route's bits.  Other rates: every clip sample
within the error bound of a T-term fp32 dot product, (T + 2) 2^-24 sum_t |taps_t x_t|, of the fp64 resampling of THAT SPAN ALONE
(a neighbouring sample of the track leaking in misses the bound by three orders of magnitude or more, tests/test_cpu_audio_track.py);
embeddings within the encoder's stated tolerance of the file route (cosine >= 1 - 5e-5, |diff| <= 2e-3 on unit rows).
Measured on an MI355X (2-block audio tower, synthetic weights): see DESIGN.md, "Audio track on the device"."""
import math

import numpy as np
import pytest
import torch

import audio_track_oracle as ato

pytestmark = pytest.mark.gpu

RATES = [44100, 48000, 22050, 8000]
COS_TOL, ABS_TOL = 5e-5, 2e-3


@pytest.fixture(scope="module")
def model():
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    return ImageBind(state_dict=synthetic_state_dict(("audio",), depth={"audio": 2}), towers=("audio",), depth={"audio": 2})


def _write_segments(audio, rate, spans, folder, tag):
    """The reference's recipe per span (hippocampal_memory.py:1205-1219): the temporary wav files it would embed."""
    from scipy.io import wavfile
    paths = []
    for i, (a, b) in enumerate(spans):
        paths.append(str(folder / f"{tag}_{i}.wav"))
        wavfile.write(paths[-1], rate, ato.reference_segment(audio, a, b))
    return paths


@pytest.fixture(scope="module")
def files16(tmp_path_factory):
    folder = tmp_path_factory.mktemp("audio_track_16k")
    out = {}
    for layout in ato.LAYOUTS:
        audio = ato.make_track(layout)
        out[layout] = (audio, _write_segments(audio, ato.SR, ato.SPANS, folder, layout))
    return out


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def _within_encoder_tolerance(got, want, what):
    g, w = _unit(got.double()), _unit(want.double())
    cos = (g * w).sum(dim=1)
    worst_cos, worst_abs = float((1 - cos).max()), float((g - w).abs().max())
    print(f"{what}: worst 1 - cos {worst_cos:.3e}, worst |diff| {worst_abs:.3e}")
    assert worst_cos <= COS_TOL and worst_abs <= ABS_TOL, what
    return worst_cos, worst_abs


# ---- 16 kHz: exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ato.LAYOUTS)
def test_16k_melspec_is_the_file_route_bit_for_bit(layout, files16):
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.preprocess import load_and_transform_audio_data_device
    audio, paths = files16[layout]
    track = AudioTrack(audio, ato.SR)
    got = track.melspec(ato.SPANS)
    want = load_and_transform_audio_data_device(paths, track.device)
    assert got.shape == want.shape == (len(ato.SPANS), 3, 1, 128, 204) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    lengths = sorted(clips.shape[1] for _, clips in track.segment_clips(ato.SPANS))
    assert lengths == [320, 20800, 31999, 32000]


def test_16k_embeddings_are_the_file_route_bit_for_bit_and_single_spans_agree(model, files16):
    from hippomm_amd.audio_track import AudioTrack
    audio, paths = files16["f64_n1"]
    track = AudioTrack(audio, ato.SR, model.device)
    got = model.extract_audio_segments(track, ato.SR, ato.SPANS)
    assert got.shape == (len(ato.SPANS), 1024) and got.dtype == torch.float32 and got.device == model.device
    assert torch.equal(got, model.forward({"audio": track.melspec(ato.SPANS)})["audio"])
    assert torch.equal(got, model.extract_features({"audio": paths}, ["audio"])["audio"])
    assert torch.equal(got, model.extract_audio_segments(audio, ato.SR, ato.SPANS))          # from the array: uploaded by the call
    # one span per call: the tower's few-row regime differs from the batched one by design, within the stated tolerance
    single = torch.cat([model.extract_audio_segments(track, ato.SR, [s]) for s in ato.SPANS])
    _within_encoder_tolerance(single, got, "16 kHz, one span per call against the batched call")
    assert model.extract_audio_segments(track, ato.SR, []).shape == (0, 1024)
    with pytest.raises(ValueError, match="16000 Hz"):
        model.extract_audio_segments(track, 44100, ato.SPANS)
    with pytest.raises(ValueError, match="empty"):
        model.extract_audio_segments(track, ato.SR, [(0, 32000), (ato.N_TRACK, ato.N_TRACK + 5)])


# ---- peaks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_span_peaks_propagate_nan_and_scale_only_above_one(dtype):
    from hippomm_amd.audio_track import AudioTrack, clip_spans
    from hippomm_amd.preprocess import _audio_clip_bounds
    rng = np.random.default_rng(3)
    x = (0.3 * rng.uniform(-1, 1, 50001)).astype(dtype)
    spans = [(101, 20101), (20101, 45000), (45001, 49999), (3, 19), (7, 50001), (10001, 15000), (20000, 20100)]
    x[5000] = np.nan                                              # in spans 0 and 4
    x[30000] = -1.0 if dtype == np.float32 else -(1.0 + 1e-12)    # span 1: the peak of the NARROWED samples is exactly 1.0
    x[46000], x[47000] = np.inf, -np.inf                          # span 2
    x[12000] = 2.5                                                # span 5: scaled
    x32 = x.astype(np.float32)
    track = AudioTrack(x, ato.SR)
    peaks = track.span_peaks(clip_spans(spans, x.shape[0])).cpu().numpy()
    want = np.array([np.abs(x32[a:b]).max() for a, b in spans], dtype=np.float32)
    assert np.isnan(want[[0, 4]]).all() and want[1] == 1.0 and np.isinf(want[2]) and want[5] == 2.5 and want[3] < 1 and want[6] < 1
    assert np.array_equal(np.isnan(peaks), np.isnan(want))
    assert np.array_equal(peaks[~np.isnan(want)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))
    got = {}
    for positions, clips in track.segment_clips(spans):
        for i, s in enumerate(positions):
            got[s] = clips[3 * i:3 * i + 3].cpu().numpy()
    for s, (a, b) in enumerate(spans):
        with np.errstate(invalid="ignore"):
            seg, p, scaled = ato.resident_segment(x32, a, b)
        assert scaled == (s in (2, 5))
        for c, (f, e) in enumerate(_audio_clip_bounds(b - a, ato.SR)):
            w, g = seg[f:e], got[s][c]
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), (s, c)
            if s == 2:
                assert nan.sum() == 2                             # inf / inf
            same = g.view(np.uint32) == w.view(np.uint32)
            assert same[~nan].all(), (s, c)
            if not scaled:
                assert same.all(), (s, c)                         # unscaled: a copy, the NaN's own bits included


# ---- other rates -------------------------------------------------------------------------------------------------------------
def _rate_case(rate, layout):
    n = 9 * rate + 13
    quiet = (int(5.0 * rate), int(7.5 * rate))
    audio = ato.make_track(layout, n=n, rate=rate, quiet=quiet, seed=rate)
    spans = [(0, int(3.37 * rate)),                              # the track's first sample
             (n - int(2.5 * rate), n),                           # its last
             (int(1.1 * rate) + 3, int(4.47 * rate) + 3),        # the middle of the loud stretch: what a leak would pick up
             (int(5.2 * rate), int(6.5 * rate)),                 # shorter than 2 s after resampling, unscaled
             (int(5.1 * rate) + 1, int(7.3 * rate))]             # 2.2 s of the quiet stretch, unscaled
    return audio, spans


@pytest.mark.parametrize("layout", ["f64_n1", "f32_n"])
@pytest.mark.parametrize("rate", RATES)
def test_other_rates_every_clip_sample_meets_the_dot_product_bound(rate, layout):
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.preprocess import _audio_clip_bounds, melspec_clips_device, resample_waveform
    audio, spans = _rate_case(rate, layout)
    x32 = ato.narrowed_track(audio)
    track = AudioTrack(audio, rate)
    groups = track.segment_clips(spans)
    got, lengths = {}, set()
    for positions, clips in groups:
        assert clips.dtype == torch.float32 and clips.shape[0] == 3 * len(positions)
        lengths.add(clips.shape[1])
        host = clips.cpu().numpy()
        for i, s in enumerate(positions):
            got[s] = host[3 * i:3 * i + 3]
    scaled_any, worst = [], 0.0
    for s, (a, b) in enumerate(spans):
        seg, p, scaled = ato.resident_segment(x32, a, b)
        scaled_any.append(scaled)
        want, mag, T = ato.resample_fp64(seg, rate)
        n16 = resample_waveform(torch.from_numpy(np.ascontiguousarray(seg))[None], rate).shape[-1]
        assert want.shape[0] == n16 == math.ceil(16000 * (b - a) / rate)
        bounds = _audio_clip_bounds(n16, 16000)
        for c, (f, e) in enumerate(bounds):
            assert got[s][c].shape == (e - f,), (s, c)
            err = np.abs(got[s][c].astype(np.float64) - want[f:e])
            limit = (T + 2) * 2.0 ** -24 * mag[f:e]
            worst = max(worst, float((err / limit).max()))
            assert np.all(err <= limit), (rate, s, c, float((err / limit).max()))
    print(f"rate {rate} {layout}: worst |err| / bound {worst:.3f}")
    assert any(scaled_any) and not all(scaled_any) and len(lengths) >= 2 and 32000 in lengths
    # the mel spectrograms are hmm_audio_fbank on exactly these clips
    mel = track.melspec(spans)
    for positions, clips in groups:
        want_mel = melspec_clips_device(clips).view(len(positions), 3, 1, 128, 204)
        assert torch.equal(mel[torch.tensor(positions, device=mel.device)], want_mel)


@pytest.mark.parametrize("rate", RATES)
def test_other_rates_embeddings_stay_within_the_encoder_tolerance_of_the_file_route(rate, model, tmp_path):
    audio, spans = _rate_case(rate, "f64_n1")
    paths = _write_segments(audio, rate, spans, tmp_path, f"r{rate}")
    want = model.extract_features({"audio": paths}, ["audio"])["audio"]
    got = model.extract_audio_segments(audio, rate, spans)
    assert got.shape == want.shape == (len(spans), 1024)
    _within_encoder_tolerance(got, want, f"{rate} Hz, device track against the wav files")


# ---- determinism and batch composition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [16000, 44100])
def test_a_span_has_the_same_clip_bits_alone_among_others_and_again(rate):
    from hippomm_amd.audio_track import AudioTrack
    audio, spans = _rate_case(rate, "f64_n1")
    track = AudioTrack(audio, rate)

    def clips_of(call_spans, which):
        for positions, clips in track.segment_clips(call_spans):
            if which in positions:
                i = positions.index(which)
                return clips[3 * i:3 * i + 3].clone()
        raise AssertionError(which)

    for s in (2, 3):
        alone = clips_of([spans[s]], 0)
        assert torch.equal(alone.view(torch.int32), clips_of(spans, s).view(torch.int32))
        assert torch.equal(alone.view(torch.int32), clips_of(list(reversed(spans)), len(spans) - 1 - s).view(torch.int32))
        assert torch.equal(alone.view(torch.int32), clips_of([spans[s]], 0).view(torch.int32))
