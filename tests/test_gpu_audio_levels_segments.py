"""GPU: sequence segmentation with the audio-level scan on the resident track (audio_track=) gives the segment list of the host
route exactly -- start and end times as floats, frames, frame_times -- audio-only and with a video walk whose cuts the audio
overrides.  The tracks have silences placed so that a walk step breaks at its last window (silence at the step's end), in its
middle, and never (no silence in reach)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SECONDS = 90


def make_audio(rate: int, layout: str, seconds: float = SECONDS, seed: int = 17) -> np.ndarray:
    """Noise at about -26 dB with silences (exact zeros, or noise at -66 dB) at 9.4-10.2 s (the last window of the first step),
    16.4-17.1 s (the middle of the next), 31-32.2 s, and 52.75-53.3 s, which covers no whole window; nothing after that, so the
    last steps never break."""
    rng = np.random.default_rng(seed)
    n = int(seconds * rate) + 7
    x = 0.05 * rng.standard_normal(n)
    for a, b, gain in ((9.4, 10.2, 0.0), (16.4, 17.1, 0.01), (31.0, 32.2, 0.0), (52.75, 53.3, 0.01)):
        x[int(a * rate):int(b * rate)] *= gain
    if layout == "f64_n1":
        return x[:, None].copy()
    other = 0.02 * rng.standard_normal(n)
    other[x == 0] = 0
    return np.stack([x + other, x - other], axis=1).astype(np.float32)          # f32 stereo


def same_segments(got, want, audio_given: bool):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert type(g.start_time) is type(w.start_time) and type(g.end_time) is type(w.end_time)
        assert float(g.start_time).hex() == float(w.start_time).hex() and float(g.end_time).hex() == float(w.end_time).hex()
        assert g.frames == w.frames and g.frame_times == w.frame_times
        if audio_given:
            assert g.audio_data.shape == w.audio_data.shape                       # the same slice of the caller's array
            assert g.audio_data.__array_interface__["data"][0] == w.audio_data.__array_interface__["data"][0]
        else:
            assert g.audio_data is None


CASES = [(8000, "f64_n1"), (44100, "f64_n1"), (8000, "f32_stereo"), (44100, "f32_stereo")]


@pytest.mark.parametrize("rate,layout", CASES)
def test_audio_only_segments_equal_the_host_routes(rate, layout):
    from hippomm_amd.audio_track import AudioTrack, spans_of
    from hippomm_amd.segmentation import segment_sequence
    audio = make_audio(rate, layout)
    want = segment_sequence(None, None, audio, rate)
    ends = [s.end_time for s in want]
    window = int(0.5 * rate) / rate
    # the three kinds of step: cut by the audio at the step's last window, cut in its middle, run to the full 10 s
    assert any(abs((e - s.start_time) - (10.0 - window)) < 1e-9 for s, e in zip(want, ends))
    assert any(5.0 < e - s.start_time < 10.0 - 2 * window for s, e in zip(want, ends))
    assert any(e - s.start_time == 10.0 for s, e in zip(want, ends))
    track = AudioTrack(audio, rate)
    same_segments(segment_sequence(None, None, audio, rate, audio_track=track), want, True)
    got = segment_sequence(None, None, None, rate, audio_track=track)
    same_segments(got, want, False)
    assert spans_of(got, rate) == [(int(s.start_time * rate), int(s.end_time * rate)) for s in want]


@pytest.mark.parametrize("rate,layout", CASES)
def test_segments_with_video_equal_the_host_routes(rate, layout):
    """A stub score_window through walk_segments: every frame pair is similar except those whose later frame is a multiple of 23,
    so the video scan cuts some steps and the audio scan, which runs after it, overrides the cut where it finds a silence."""
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.segmentation import walk_segments
    audio = make_audio(rate, layout)
    frame_times = [0.5 * k for k in range(2 * SECONDS - 10)]      # the video ends before the audio does
    frames = [f"frame_{k:04d}.jpg" for k in range(len(frame_times))]

    def score_window(pairs):
        for later, _ in pairs:
            yield 0.5 if later % 23 == 0 else 0.99

    want = walk_segments(frames, frame_times, audio, rate, score_window)
    assert len({len(s.frames) for s in want}) > 2
    track = AudioTrack(audio, rate)
    same_segments(walk_segments(frames, frame_times, audio, rate, score_window, audio_track=track), want, True)
    same_segments(walk_segments(frames, frame_times, None, rate, score_window, audio_track=track), want, False)


@pytest.mark.parametrize("rate,layout", [(8000, "f64_n1"), (44100, "f32_stereo")])
def test_a_track_shorter_than_the_frame_times_imply(rate, layout):
    """The walk's windows run past the end of the audio: clipped and empty windows, whose host level is -100, decide as on the host."""
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.segmentation import walk_segments
    import warnings
    audio = make_audio(rate, layout, seconds=23.3)
    frame_times = [0.5 * k for k in range(81)]                    # 40 s of video
    frames = [f"frame_{k:04d}.jpg" for k in range(len(frame_times))]

    def score_window(pairs):
        for _ in pairs:
            yield 0.99

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # numpy's "Mean of empty slice" on the host route
        want = walk_segments(frames, frame_times, audio, rate, score_window)
    track = AudioTrack(audio, rate)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)            # the resident route reproduces the values, not the warnings
        got = walk_segments(frames, frame_times, audio, rate, score_window, audio_track=track)
    same_segments(got, want, True)


def test_mismatching_rate_or_length_raises_and_the_drop_in_forwards_the_track():
    from types import SimpleNamespace
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.segmentation import _segment_sequence, segment_sequence, walk_segments
    audio = make_audio(8000, "f64_n1", seconds=21.0)
    track = AudioTrack(audio, 8000)
    with pytest.raises(ValueError, match="8000 Hz"):
        segment_sequence(None, None, audio, 16000, audio_track=track)
    with pytest.raises(ValueError, match="8000 Hz"):
        walk_segments(None, None, None, None, None, audio_track=track)
    with pytest.raises(ValueError, match="samples"):
        segment_sequence(None, None, audio[:-1], 8000, audio_track=track)
    want = segment_sequence(None, None, audio, 8000)
    memory = SimpleNamespace(max_segment_duration=10.0, min_segment_duration=5.0, frame_similarity_threshold=0.95,
                             audio_silence_threshold=-40)
    same_segments(_segment_sequence(memory, None, None, audio, 8000, audio_track=track), want, True)
    memory.audio_track = track
    same_segments(_segment_sequence(memory, None, None, None, 8000), want, False)
