"""CPU: tempo and pitch on the host -- `wave_codec.wsola_pcm16` / `shift_pcm16` against the plain-integer restatement of
tests/prosody_ref.py, the exact laws (lengths, identity through the search, the window file the library builds in), an analytic check on
sines against no code of ours, the refusals character for character, and the `tempo` / `pitch` options through `WaveSpec`,
`check_request_options`, `finish_requests`, the manager and the routes."""
import base64
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import prosody_ref as ref
from tts_indic_server_f5_amd import infer, serve, wave_codec

from test_script_host import RA, RB, SCRIPT, NoiseModel, Vocoder, _wav, B  # noqa: E402
from test_script_host import client as script_client  # noqa: E402,F401  (a manager without a model behind a TestClient)
from test_wave_encode_host import TEXT, _voice, client  # noqa: E402,F401  (the stand-in manager behind a TestClient)

RATE = 24000
L, H, D = 960, 480, 240
LENGTHS = [0, 1, 2, 239, 479, 480, 481, 959, 960, 961, 1441, 5000]
STRETCHES = [(2, 1), (1, 2), (100, 99), (99, 100), (18, 17), (29, 41), (37, 55)]
# the same stretches as (tempo, pitch) where hundredths of a tempo reach them: 99/100 is a tempo of 1.0101...
SHIFTS = {(2, 1): (0.5, 0), (1, 2): (2.0, 0), (100, 99): (0.99, 0), (18, 17): (1.0, 1), (29, 41): (1.0, -6), (37, 55): (1.25, -3)}
CONTENTS = ("zeros", "floor", "alternating", "square100", "noise")
DEFAULTS = dict(speed=1.0, nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=None)


def _content(kind, n):
    t = np.arange(n)
    if kind == "zeros":
        return np.zeros(n, dtype=np.int16)
    if kind == "floor":
        return np.full(n, -32768, dtype=np.int16)
    if kind == "alternating":                                            # full scale: every difference is 65535 or 0
        return np.where(t % 2 == 0, 32767, -32768).astype(np.int16)
    if kind == "square100":                                              # a period of 240 samples = D: candidates a period apart tie exactly
        return np.where((t // 120) % 2 == 0, 12000, -12000).astype(np.int16)
    return infer.quantise_pcm16(0.2 * np.random.default_rng(n).standard_normal(n))


# ------------------------------------------------------------------------------------------------ the definition
def test_window_and_constants():
    W = wave_codec.wsola_window()
    assert (wave_codec.PROSODY_FRAME, wave_codec.PROSODY_HOP, wave_codec.PROSODY_SEARCH) == (L, H, D)
    assert W.dtype == np.int64 and len(W) == L and W is wave_codec.wsola_window() and not W.flags.writeable
    assert W.tolist() == ref.window()
    assert np.array_equal(W[:H] + W[H:], np.full(H, 32768)) and W[0] == 0 and W[H - 1] == 32768 and (np.diff(W[:H]) >= 0).all()
    assert wave_codec.PROSODY_OPTIONS == ("tempo", "pitch") and infer.REQUEST_OPTIONS[-2:] == ("tempo", "pitch")
    assert set(infer.REQUEST_OPTIONS[6:11]) == set(wave_codec.DELIVERY_OPTIONS) and len(wave_codec.DELIVERY_OPTIONS) == 5
    assert sorted(wave_codec.PITCH_RATIOS) == [s for s in range(-6, 7) if s]
    for s, (p, q) in wave_codec.PITCH_RATIOS.items():
        assert wave_codec.PITCH_RATIOS[-s] == (q, p) and (p, q) == (ref.ratio(s).numerator, ref.ratio(s).denominator)
        assert abs(1200.0 * np.log2(p / q) - 100.0 * s) < 2.0, s           # within 2 cents of the equal-tempered step
        of, nf, width, rows = wave_codec.rate_pair(p, q)
        assert (of, nf) == (p, q) and 4 * nf * rows < 11 * 1024, s         # its tap table stays below 11 KB


def test_the_library_builds_in_the_same_window():
    csrc = os.path.join(os.path.dirname(os.path.abspath(infer.__file__)), "csrc")
    body = "".join(line for line in open(os.path.join(csrc, "wsola_window.inc"), encoding="utf-8") if not line.startswith("//"))
    assert [int(v) for v in re.findall(r"-?\d+", body)] == [int(v) for v in wave_codec.wsola_window()[:H]] == ref.window()[:H]
    core = open(os.path.join(csrc, "wave_prosody_core.h"), encoding="utf-8").read()
    assert f"kPrFrame = {L}, kPrHop = {H}, kPrSearch = {D};" in core
    ps = ", ".join(str(wave_codec.PITCH_RATIOS[s][0]) for s in range(1, 7))
    qs = ", ".join(str(wave_codec.PITCH_RATIOS[s][1]) for s in range(1, 7))
    assert f"kPrPitchP[kPrPitchMax] = {{{ps}}}, kPrPitchQ[kPrPitchMax] = {{{qs}}};" in core


@pytest.mark.parametrize("stretch", STRETCHES, ids=lambda s: f"{s[0]}_{s[1]}")
def test_wsola_equals_the_restatement(stretch):
    """Every length, every content: the samples and every frame start of the plain-integer restatement."""
    P, Q = stretch
    for n in LENGTHS:
        for kind in CONTENTS:
            x = _content(kind, n)
            y, s = wave_codec._wsola_frames(x, P, Q)
            want_y, want_s = ref.wsola(x.tolist(), P, Q)
            assert y.dtype == np.int16 and s == want_s and y.tolist() == want_y, (n, kind)
            assert np.array_equal(wave_codec.wsola_pcm16(x, P, Q), y)


def test_exact_ties_go_to_the_smaller_then_the_negative_offset():
    """On the 100 Hz square, candidates a period (240 samples) apart cost the same: among the offsets of least cost, worked out here frame by
    frame, the one chosen has the least |d|, and of -d and d the negative one.  On zeros every cost ties at 0 and every offset is 0."""
    tied = both_signs = 0
    for P, Q in STRETCHES:
        x = _content("square100", 5000)
        xt = np.concatenate([np.zeros(2000, dtype=np.int64), x.astype(np.int64), np.zeros(4000, dtype=np.int64)])
        _, s = wave_codec._wsola_frames(x, P, Q)
        for k in range(1, len(s)):
            p, t = (k * H * Q) // P - H, s[k - 1] + H
            cost = [int(np.abs(xt[2000 + p + d:2000 + p + d + L] - xt[2000 + t:2000 + t + L]).sum()) for d in range(-D, D + 1)]
            least = [d for d in range(-D, D + 1) if cost[d + D] == min(cost)]
            tied += len(least) > 1
            both_signs += any(-d in least for d in least if d > 0)
            assert s[k] - p == min(least, key=lambda d: (abs(d), d)), (P, Q, k, least)
        _, s = wave_codec._wsola_frames(np.zeros(5000, dtype=np.int16), P, Q)
        assert s == [(k * H * Q) // P - H for k in range(len(s))]
    assert tied >= 10 and both_signs >= 1, (tied, both_signs)
    assert [int(wave_codec.wsola_rank(np.int64(d))) for d in (0, -1, 1, -2, 2, -240, 240)] == [0, 1, 2, 3, 4, 479, 480]


@pytest.mark.parametrize("stretch", sorted(SHIFTS), ids=lambda s: f"{s[0]}_{s[1]}")
def test_shift_equals_the_restatement(stretch):
    tempo, pitch = SHIFTS[stretch]
    hundredths = round(100 * tempo)
    assert ref.stretch(hundredths, pitch) == stretch == wave_codec.prosody_stretch(hundredths, pitch)
    taps = width = None
    if pitch:
        _, _, width, table = wave_codec.resample_taps(*wave_codec.PITCH_RATIOS[pitch])
        taps = table.numpy().astype(np.float64).tolist()
    for n in LENGTHS:
        for kind in CONTENTS:
            x = _content(kind, n)
            got = wave_codec.shift_pcm16(x, tempo, pitch)
            assert got.dtype == np.int16 and got.tolist() == ref.shift(x.tolist(), hundredths, pitch, taps, width), (n, kind)
            assert len(got) == wave_codec.shifted_length(n, stretch, pitch)


def test_length_laws():
    for n in LENGTHS + [30011, 3 * RATE]:
        for P, Q in STRETCHES:
            x = np.zeros(n, dtype=np.int16)
            assert len(wave_codec.wsola_pcm16(x, P, Q)) == -(-n * P // Q)
        for hundredths in (50, 80, 99, 125, 133, 200):
            got = wave_codec.shift_pcm16(np.zeros(n, dtype=np.int16), hundredths / 100)
            assert len(got) == -(-n * 100 // hundredths)                 # the duration divided by the tempo
        for s in (-6, -1, 1, 5, 6):
            p, q = wave_codec.PITCH_RATIOS[s]
            got = wave_codec.shift_pcm16(np.zeros(n, dtype=np.int16), None, s)
            assert len(got) == -(-q * -(-n * p // q) // p) and 0 <= len(got) - n <= 1 + q // p   # the duration kept, up to the two ceilings


def test_identity_through_the_search():
    """P == Q: cost 0 at offset 0, which the tie rule prefers, so the private entry gives the input back sample for sample; the public one
    returns the input object, and so does `shift_pcm16` for neutral options."""
    for n in LENGTHS:
        for kind in CONTENTS:
            x = _content(kind, n)
            for P in (1, 7):
                y, s = wave_codec._wsola_frames(x, P, P)
                assert np.array_equal(y, x) and s == [k * H - H for k in range(len(s))], (n, kind)
            assert wave_codec.wsola_pcm16(x, 3, 3) is x
            for neutral in ((None, None), (1.0, 0), (1, None), (None, 0)):
                assert wave_codec.shift_pcm16(x, *neutral) is x


def test_output_never_leaves_int16_at_full_scale():
    for kind in ("floor", "alternating"):
        for P, Q in STRETCHES:
            y = wave_codec.wsola_pcm16(_content(kind, 5000), P, Q)
            assert y.dtype == np.int16 and int(y.min()) >= -32768 and int(y.max()) <= 32767
    assert (wave_codec.wsola_pcm16(_content("floor", 5000), 2, 1)[H:-2 * L] == -32768).all()   # away from the edges a constant stays one


def _analyse(y):
    """(peak frequency in Hz, rms) of a wave: a Hann window, a 2^20-point FFT, 2400 samples dropped at each edge."""
    y = y[2400:len(y) - 2400].astype(np.float64)
    spectrum = np.abs(np.fft.rfft(y * np.hanning(len(y)), 1 << 20))
    return float(np.argmax(spectrum)) * RATE / (1 << 20), float(np.sqrt(np.mean(y * y)))


def _overlap_add(x, P, Q):
    """The same frames and window WITHOUT the search (every offset 0): what the bounds below must tell from WSOLA."""
    n = len(x)
    m = -(-n * P // Q)
    xt = np.zeros(n + 4000, dtype=np.int64)
    xt[1000:1000 + n] = x
    s = np.array([(k * H * Q) // P - H for k in range(-(-m // H) + 1)])
    W = wave_codec.wsola_window()
    at = s[:, None] + np.arange(H)[None] + 1000
    return ((W[H:] * xt[at[:-1] + H] + W[:H] * xt[at[1:]] + 16384) >> 15).reshape(-1)[:m].astype(np.int16)


@pytest.mark.parametrize("freq", [220, 1000])
def test_sines_keep_their_frequency_under_tempo_and_move_by_the_ratio_under_pitch(freq):
    """Against no code of ours: a 2 s sine of amplitude 8000 keeps its spectral peak under a tempo (0.8, 1.25, 2.0), has it at f p / q
    under a pitch (+1, -1, +3, +6, -6), and keeps its rms in both cases.  Bounds: 1 Hz and 1 %.

    Measured on the host function: the peak is off by at most 0.085 Hz (220 Hz, pitch +6) and the rms by at most 0.042 % (220 Hz, pitch -1
    and +3).  Plain overlap-add without the search, on the 220 Hz sine: 4.99 to 20.01 Hz off and 2.42 to 25.99 % of the rms lost under the
    tempos, 6.33 to 20.35 Hz and 7.37 to 17.94 % under the pitches -- so the bounds separate the two by a factor of five each way or more.
    (At 1000 Hz, whose period divides every hop here, overlap-add keeps a tempo's sine too; it is asserted to fail at 220 Hz only.)"""
    x = np.rint(8000.0 * np.sin(2 * np.pi * freq * np.arange(2 * RATE) / RATE)).astype(np.int16)
    f0, rms0 = _analyse(x)
    assert abs(f0 - freq) < 0.05
    cases = [(t, 0) for t in (0.8, 1.25, 2.0)] + [(1.0, s) for s in (1, -1, 3, 6, -6)]
    for tempo, pitch in cases:
        p, q = wave_codec.PITCH_RATIOS[pitch] if pitch else (1, 1)
        f, rms = _analyse(wave_codec.shift_pcm16(x, tempo, pitch))
        print(f"{freq} Hz, tempo {tempo}, pitch {pitch}: peak {f - freq * p / q:+.3f} Hz, rms {100 * (rms / rms0 - 1):+.3f} %")
        assert abs(f - freq * p / q) <= 1.0 and abs(rms / rms0 - 1.0) <= 0.01, (tempo, pitch, f, rms / rms0)
        if freq == 220:                                                  # the bounds have teeth: the same frames without the search miss both
            y = _overlap_add(x, *wave_codec.prosody_stretch(round(100 * tempo), pitch))
            f, rms = _analyse(wave_codec._polyphase_whole(y, *wave_codec.pitch_taps(pitch)) if pitch else y)
            assert abs(f - freq * p / q) > 1.0 and abs(rms / rms0 - 1.0) > 0.01, (tempo, pitch, f, rms / rms0)


# ------------------------------------------------------------------------------------------------ the options
def test_refusals_character_for_character():
    for bad in (True, False, "1.0", 0.49, 2.01, 0.505, 1.0000001, float("nan"), float("inf"), [1.0], 0, 3):
        with pytest.raises(ValueError) as e:
            infer.WaveSpec.of(dict(tempo=bad))
        assert str(e.value) == f"tempo must be a number from 0.5 to 2 in steps of 0.01 (got {bad!r})"
        with pytest.raises(ValueError, match="tempo must be"):
            wave_codec.shift_pcm16(np.zeros(4, dtype=np.int16), bad)
    for bad in (True, False, 2.0, 1.5, "2", -7, 7, [1]):
        with pytest.raises(ValueError) as e:
            infer.WaveSpec.of(dict(pitch=bad))
        assert str(e.value) == f"pitch must be a whole number of semitones from -6 to 6 (got {bad!r})"
    for tempo, pitch, P, Q in ((0.5, 6, 82, 29), (0.5, 1, 36, 17), (2.0, -1, 17, 36), (1.5, -6, 58, 123), (0.7, 6, 410, 203)):
        with pytest.raises(ValueError) as e:
            infer.WaveSpec.of(dict(tempo=tempo, pitch=pitch))
        assert str(e.value) == f"tempo {tempo} with pitch {pitch} stretches the wave by {P}/{Q}: outside 1/2 to 2"
        assert P > 2 * Q or Q > 2 * P
    for ok in (0.5, 2, 2.0, 1, 0.58, 0.07 * 10, 1.1, np.float32(1.25), np.int64(2)):     # (0.58 and 0.07 * 10 are not exact hundredths in binary)
        assert infer.WaveSpec.of(dict(tempo=ok)).tempo == round(100 * float(ok)) / 100
    assert infer.WaveSpec.of(dict(pitch=np.int32(-6))).pitch == -6 and isinstance(infer.WaveSpec.of(dict(pitch=np.int32(-6))).pitch, int)
    # the new options are checked after the existing three: every pinned refusal keeps its message
    with pytest.raises(ValueError, match="loudness must be"):
        infer.WaveSpec.of(dict(loudness=True, tempo=True))
    with pytest.raises(ValueError, match="flac_level needs encoding"):
        infer.WaveSpec.of(dict(flac_level=1, pitch=9))
    with pytest.raises(ValueError, match="sample_rate must be one of"):
        infer.WaveSpec.of(dict(sample_rate=7, tempo=9))
    for P, Q in ((0, 1), (1, 0), (True, 1), (1.0, 1), (3, 1), (1, 3), (201, 100)):
        with pytest.raises(ValueError, match="wsola_pcm16"):
            wave_codec.wsola_pcm16(np.zeros(4, dtype=np.int16), P, Q)
    with pytest.raises(ValueError, match="int16"):
        wave_codec.shift_pcm16(np.zeros(4, dtype=np.float32), 1.25)


def test_wave_spec_fields_and_the_whole_wave_rule():
    names = [f.name for f in dataclasses.fields(infer.WaveSpec)]
    assert names == list(wave_codec.DELIVERY_OPTIONS) + ["tempo", "pitch", "watermark", "keep_formants"]
    spec = infer.WaveSpec(True, -16.0, 8000, "mulaw", 0)                 # the five-argument positional form keeps its meaning
    assert (spec.tempo, spec.pitch, spec.prosody) == (1.0, 0, False) and spec == infer.WaveSpec.of(dict(remove_silence=True, loudness=-16.0, sample_rate=8000,
                                                                                                       encoding="mulaw"))
    assert infer.WaveSpec.of({}) == infer.WaveSpec() and not infer.WaveSpec().needs_whole_wave()
    assert infer.WaveSpec.of(dict(tempo=1.0, pitch=0)) == infer.WaveSpec() == infer.WaveSpec.of(dict(tempo=None, pitch=None))
    for opts, stretch in ((dict(tempo=1.25), (4, 5)), (dict(pitch=2), (46, 41)), (dict(tempo=0.9, pitch=-6), (290, 369))):
        spec = infer.WaveSpec.of(opts)
        assert spec.prosody and spec.needs_whole_wave() and spec.needs_whole_wave(streamed=True)
        assert spec.whole_wave_message() == infer.WHOLE_WAVE_PROSODY
        assert spec.stretch == wave_codec.prosody_stretch(round(100 * spec.tempo), spec.pitch) and spec.stretch[0] * stretch[1] == spec.stretch[1] * stretch[0]
    assert infer.WHOLE_WAVE_PROSODY == ("tempo and pitch are applied to the request's whole wave: they are not available for a list of chunk texts, "
                                        "on a streaming path or with join=False")
    # prosody is the message only when it is the sole reason; otherwise the existing rule picks it
    assert infer.WaveSpec.of(dict(tempo=1.25, loudness=-16.0)).whole_wave_message() == infer.WHOLE_WAVE_LOUDNESS
    assert infer.WaveSpec.of(dict(tempo=1.25, remove_silence=True)).whole_wave_message() == infer.WHOLE_WAVE
    assert infer.WaveSpec.of(dict(pitch=1, sample_rate=8000)).whole_wave_message() == infer.WHOLE_WAVE
    assert infer.needs_whole_wave(dict(pitch=1), streamed=True) and infer.whole_wave_message(dict(pitch=1)) == infer.WHOLE_WAVE_PROSODY


def test_check_request_options_and_the_route_models():
    check = serve.check_request_options
    assert check(dict(tempo=1.25, pitch=-2)) == dict(tempo=1.25, pitch=-2)
    assert check(dict(tempo=1.0, pitch=0, speed=None)) == {} and check(dict(tempo=1, pitch=None)) == {}    # what a request gets anyway is dropped
    assert check(dict(tempo=0.58)) == dict(tempo=0.58) and isinstance(check(dict(tempo=2))["tempo"], float)
    with pytest.raises(ValueError, match="tempo must be a number from 0.5 to 2"):
        check(dict(tempo=True))
    with pytest.raises(ValueError, match="pitch must be a whole number"):
        check(dict(pitch=2.0))
    with pytest.raises(ValueError, match="outside 1/2 to 2"):
        check(dict(tempo=0.5, pitch=3))
    for name in infer.PROSODY_OPTIONS:
        with pytest.raises(ValueError, match="unknown option"):            # not on the edit route: its options are pinned
            check({name: 1}, allowed=tuple(dict.fromkeys(serve.EDIT_OPTIONS + serve.EDIT_DELIVERY)))
    assert not set(infer.PROSODY_OPTIONS) & set(serve.EDIT_DELIVERY)
    assert serve.stream_refusal(dict(tempo=1.25)) == serve.STREAM_PROSODY == serve.stream_refusal(dict(pitch=-1, sample_rate=8000))
    assert serve.stream_refusal(dict(tempo=1.25, loudness=-16.0)) == serve.STREAM_LOUDNESS
    assert serve.stream_refusal(dict(tempo=1.25, remove_silence=True)) == serve.STREAM_REMOVE_SILENCE and serve.stream_refusal(dict(sample_rate=8000)) is None
    assert serve.STREAM_PROSODY == "tempo and pitch are applied to the request's whole wave: they are not available on a streaming path"
    models = serve.request_models()
    for model in (models.KannadaSynthesizeRequest, models.SynthesizeRequest, models.CloneRequest, models.ScriptRequest):
        assert {"tempo", "pitch"} <= set(model.model_fields) and set(infer.REQUEST_OPTIONS) <= set(model.model_fields), model
    assert not {"tempo", "pitch"} & set(models.EditRequest.model_fields)


def test_finish_pcm16_is_the_composition_with_the_new_step():
    rng = np.random.default_rng(5)
    speech = infer.quantise_pcm16(0.1 * rng.standard_normal(RATE))
    pause = np.concatenate([speech, np.zeros(int(2.5 * RATE), dtype=np.int16), speech[::-1]])
    cut = infer.remove_silence_pcm(pause, RATE)
    assert len(cut) < len(pause)
    option_sets = [dict(tempo=1.25), dict(pitch=-2), dict(tempo=0.8, pitch=3, remove_silence=True), dict(tempo=1.5, loudness=-20.0),
                   dict(pitch=1, sample_rate=8000, encoding="mulaw"), dict(tempo=1.1, pitch=-1, encoding="flac", flac_level=1, loudness=-23.0, remove_silence=True),
                   dict(loudness=-23.0, sample_rate=8000, encoding="mulaw", remove_silence=True)]
    for opts in option_sets:
        spec = infer.WaveSpec.of(opts)
        x = cut if spec.remove_silence else pause
        y = wave_codec.shift_pcm16(x, spec.tempo, spec.pitch)
        assert (y is x) == (not spec.prosody)
        want = infer.deliver_pcm16(infer.normalise_loudness_pcm16(y, spec.loudness), *spec.format, flac_level=spec.flac_level if spec.flac else None)
        got = infer.finish_pcm16(pause, spec)
        assert got.dtype == want.dtype and np.array_equal(got, want), opts
    # loudness is measured on what is delivered: after the stretch, not before
    spec = infer.WaveSpec.of(dict(tempo=2.0, loudness=-20.0))
    assert not np.array_equal(infer.finish_pcm16(pause, spec), wave_codec.shift_pcm16(infer.normalise_loudness_pcm16(pause, -20.0), 2.0))


def test_finish_requests_takes_the_options_per_request():
    fade = infer.cross_fade_duration
    rng = np.random.default_rng(9)
    reqs = [[(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens] for lens in ([20000], [15000, 14000], [9000])]
    texts, flags = ["x"] * 3, [False] * 3
    plain = infer.finish_requests(reqs, texts, fade, flags, want="pcm16")
    got = infer.finish_requests(reqs, texts, fade, flags, tempo=[1.25, None, 0.8], pitch=[None, 2, -1])
    for g, x, (t, s) in zip(got, plain, ((1.25, None), (None, 2), (0.8, -1))):
        assert g.dtype == np.int16 and np.array_equal(g, wave_codec.shift_pcm16(x, t, s))
    one = infer.finish_requests(reqs, texts, fade, flags, tempo=1.1)                   # one value for all
    assert all(np.array_equal(g, wave_codec.shift_pcm16(x, 1.1)) for g, x in zip(one, plain))
    today = infer.finish_requests(reqs, texts, fade, flags)
    neutral = infer.finish_requests(reqs, texts, fade, flags, tempo=1.0, pitch=0)
    assert all(a.dtype == b.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(today, neutral))   # neutral: today's bytes
    waves = infer.SegmentedWaves([reqs[1], reqs[2]], RATE // 2)                       # a script is shifted as one joined wave
    joined = infer.quantise_pcm16(infer.join_segments([reqs[1], reqs[2]], fade, RATE // 2))
    assert np.array_equal(infer.finish_requests([waves], ["x"], fade, [False], tempo=0.9, pitch=1)[0], wave_codec.shift_pcm16(joined, 0.9, 1))
    with pytest.raises(ValueError, match="tempo must be"):
        infer.finish_requests(reqs, texts, fade, flags, tempo=3.0)
    with pytest.raises(ValueError) as e:
        infer.finish_requests([reqs[0]], [["head"]], fade, pitch=2)                    # a list of chunk texts
    assert str(e.value) == infer.WHOLE_WAVE_PROSODY


def test_chunk_texts_are_refused_by_the_planner(tmp_path):
    voice = infer.PreparedVoice(_voice(tmp_path))
    plan = lambda text, opts: infer.plan_request((voice, "reference words", text, opts), DEFAULTS, target_rms=0.1, fix_duration=None, device=None,   # noqa: E731
                                                 tokenizer=infer.text_to_tokens)
    for opts in (dict(tempo=1.25), dict(pitch=-3)):
        for text in (["one chunk.", "another chunk."], ("one chunk.",)):
            with pytest.raises(ValueError) as e:
                plan(text, opts)
            assert str(e.value) == infer.WHOLE_WAVE_PROSODY
    assert plan("some text.", dict(tempo=1.25, pitch=1)).spec == infer.WaveSpec(tempo=1.25, pitch=1)
    with pytest.raises(ValueError, match="pitch must be"):
        plan("text.", dict(pitch=True))


def test_manager_and_speech_routes(client, tmp_path):
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    pcm = infer.quantise_pcm16(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text))
    want = wave_codec.shift_pcm16(pcm, 1.25, -2)
    got = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, tempo=1.25, pitch=-2)
    assert got.dtype == np.int16 and np.array_equal(got, want) and abs(len(want) - len(pcm) / 1.25) <= 2
    assert np.array_equal(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, tempo=1.0, pitch=0), mgr.synthesize(TEXT, voice.audio_path, voice.ref_text))
    raw = open(_voice(tmp_path), "rb").read()
    clip_pcm = infer.quantise_pcm16(mgr.synthesize_clip(TEXT, raw, "reference words"))
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words", pitch=3), wave_codec.shift_pcm16(clip_pcm, None, 3))
    for stream in (mgr.synthesize_stream, lambda *a, **kw: mgr.synthesize_clip_stream(TEXT, raw, "reference words", **kw)):
        for opts in (dict(tempo=0.8), dict(pitch=1)):
            with pytest.raises(ValueError) as e:
                stream(TEXT, voice.audio_path, voice.ref_text, **opts)
            assert str(e.value) == serve.STREAM_PROSODY
    body = dict(text=TEXT, tempo=1.25, pitch=-2)
    clone = dict(body, ref_audio=base64.b64encode(raw).decode(), ref_text="reference words")
    for route, extra in (("/v1/audio/speech", body), ("/v1/audio/speech/voice", dict(body, ref_audio_name="KAN_F (Happy)")), ("/v1/audio/speech/clone", clone)):
        r = c.post(route, json=dict(extra, response_format="pcm"))
        assert r.status_code == 200 and r.content == (want if "clone" not in route else wave_codec.shift_pcm16(clip_pcm, 1.25, -2)).tobytes(), route
        r = c.post(route, json=dict(extra, stream=True))
        assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_PROSODY, route
        for bad in (dict(tempo=True), dict(tempo=2.5), dict(pitch=2.0), dict(pitch=7), dict(tempo=0.5, pitch=6)):
            r = c.post(route, json=dict(extra, **bad))
            assert r.status_code == 400 and ("tempo" in r.json()["detail"] or "pitch" in r.json()["detail"]), (route, bad)
    r = c.post("/v1/audio/speech", json=dict(body, sample_rate=8000, encoding="mulaw", loudness=-20.0, response_format="pcm"))
    assert r.status_code == 200 and r.content == infer.deliver_pcm16(infer.normalise_loudness_pcm16(want, -20.0), 8000, "mulaw").tobytes()
    r = c.post("/v1/audio/speech", json=dict(text=TEXT, tempo=1.0, pitch=0, stream=True))                   # neutral: streams as today
    assert r.status_code == 200


def test_script_route_and_method(script_client):
    c, mgr, path = script_client
    mgr.load(NoiseModel(), Vocoder())
    voices = dict(main=dict(ref_audio_path=path, ref_text=RA), town=dict(ref_audio=_wav(B), ref_text=RB))
    pcm = infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4))
    want = wave_codec.shift_pcm16(pcm, 0.9, 2)
    got = mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4, tempo=0.9, pitch=2)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    with pytest.raises(ValueError) as e:
        mgr.synthesize_script_stream(SCRIPT, voices, tempo=0.9)
    assert str(e.value) == serve.STREAM_PROSODY
    town = dict(ref_audio=base64.b64encode(_wav(B)).decode(), ref_text=RB)
    body = dict(text=SCRIPT, voices=dict(main=dict(ref_audio_name="KAN_F (Happy)"), town=town), seed=4, gap=0.5, tempo=0.9, pitch=2)
    r = c.post("/v1/audio/speech/script", json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
    calls = len(mgr.model_obj.calls)
    r = c.post("/v1/audio/speech/script", json=dict(body, stream=True))
    assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_PROSODY
    r = c.post("/v1/audio/speech/script", json=dict(body, pitch=9))
    assert r.status_code == 400 and "pitch must be" in r.json()["detail"]
    assert len(mgr.model_obj.calls) == calls                                            # neither reached the sampler


def test_the_edit_method_does_not_take_the_options():
    """`serve.EDIT_DELIVERY` is pinned: an edit keeps the recording's timing and pitch."""
    assert not {"tempo", "pitch"} & set(inspect.signature(serve.TTSManager.edit).parameters)
    with pytest.raises(TypeError):
        serve.TTSManager.edit(None, b"", "x", [[0, 1]], tempo=1.25)
