"""CPU: the formant-preserving pitch shift on the host -- `wave_codec.psola_pcm16` against the plain-integer restatement of
tests/formant_ref.py on the case matrix, the exact laws (length, zeros, the unvoiced identity, the window file the library builds in),
property tests on synthetic vowels against no code of ours (the fundamental moves by p / q, the first formant stays), and the
`keep_formants` option through `shift_pcm16`, `finish_pcm16`, `check_request_options`, `finish_requests`, the manager and the routes."""
import base64
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import formant_ref as ref
from tts_indic_server_f5_amd import infer, serve, wave_codec

from test_script_host import RA, RB, SCRIPT, NoiseModel, Vocoder, _wav, B  # noqa: E402
from test_script_host import client as script_client  # noqa: E402,F401  (a manager without a model behind a TestClient)
from test_wave_encode_host import TEXT, _voice, client  # noqa: E402,F401  (the stand-in manager behind a TestClient)

RATE = 24000
LENGTHS = [0, 1, 119, 480, 1000, 24000, 30011]
CONTENTS = ("zeros", "noise", "square", "vowel", "mixed")
STEPS = [s for s in range(-6, 7) if s]
DEFAULTS = dict(speed=1.0, nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=None)
_cache: dict = {}


def _resonate(e):
    """An excitation through two-pole resonators at 700 / 1200 / 2600 Hz with bandwidths 80 / 100 / 120 Hz, in fp64."""
    y = np.asarray(e, dtype=np.float64)
    for fc, bw in ((700.0, 80.0), (1200.0, 100.0), (2600.0, 120.0)):
        r = np.exp(-np.pi * bw / RATE)
        c1, c2 = 2.0 * r * np.cos(2.0 * np.pi * fc / RATE), -r * r
        out, y1, y2 = np.empty(len(y)), 0.0, 0.0
        for j, v in enumerate(y.tolist()):
            w = v + c1 * y1 + c2 * y2
            y2, y1 = y1, w
            out[j] = w
        y = out
    return y


def vowel(n, f0, f1=None, peak=12000):
    """An impulse train (f0 Hz, gliding to f1 when given) through the resonators, its largest magnitude at `peak`: int16 [n]."""
    key = ("vowel", n, f0, f1, peak)
    if key not in _cache:
        if f1 is None:                                                   # whole-number arithmetic: an integer period stays one
            e = np.diff((np.arange(n + 1, dtype=np.int64) * int(f0)) // RATE) > 0
        else:
            e = np.diff(np.floor(np.cumsum(np.linspace(float(f0), float(f1), n) / RATE)), prepend=0.0) > 0
        y = _resonate(e.astype(np.float64))
        top = np.abs(y).max() if n else 0.0
        _cache[key] = np.rint(y * (peak / top)).astype(np.int16) if top > 0 else np.zeros(n, dtype=np.int16)
    return _cache[key]


def noise(n, sigma=2000.0, seed=0):
    return np.clip(np.rint(np.random.default_rng(seed + n).normal(0.0, sigma, n)), -32768, 32767).astype(np.int16)


def content(kind, n):
    """The case matrix's waves: int16 [n]."""
    if kind == "zeros":
        return np.zeros(n, dtype=np.int16)
    if kind == "noise":
        return noise(n)
    if kind == "square":                                                 # full scale, a period of 160 samples: exact ties in d and in the peak search
        return np.where((np.arange(n) // 80) % 2 == 0, 32767, -32768).astype(np.int16)
    if kind == "vowel":
        return vowel(n, 130)
    parts = [n // 8, n // 4, n // 4, n // 8]                             # silence, vowel, noise, silence, then a 200 -> 140 Hz glide
    last = n - sum(parts)
    return np.concatenate([np.zeros(parts[0], dtype=np.int16), vowel(parts[1], 110), noise(parts[2], 3000.0, 7), np.zeros(parts[3], dtype=np.int16),
                           vowel(last, 200, 140)])


def reference(kind, n):
    """The restatement's analysis of a case, once: (samples as a list, the track, the analysis marks)."""
    key = ("ref", kind, n)
    if key not in _cache:
        x = content(kind, n).tolist()
        frames = ref.track(x)
        _cache[key] = (x, frames, ref.analysis_marks(x, frames))
    return _cache[key]


# ------------------------------------------------------------------------------------------------ the definition
def test_window_and_constants():
    M = wave_codec.psola_window()
    assert (wave_codec.PSOLA_HOP, wave_codec.PSOLA_WINDOW, wave_codec.PSOLA_LAG_MIN, wave_codec.PSOLA_LAG_MAX) == (ref.HOP, ref.WIN, ref.LAG_MIN, ref.LAG_MAX)
    assert (wave_codec.PSOLA_MIN_ADVANCE, wave_codec.PSOLA_TABLE) == (ref.MIN_ADVANCE, ref.TABLE) == (24, 1024)
    assert M.dtype == np.int64 and len(M) == 1025 and M is wave_codec.psola_window() and not M.flags.writeable
    assert M.tolist() == ref.window() and M[0] == 32768 and M[512] == 16384 and M[1024] == 0 and (np.diff(M) <= 0).all()
    assert (M[:1022] >= 1).all() and M[1022] == 0                       # every offset inside a grain of T <= 400 weighs: (|k| 1024) // T <= 1021
    assert all((k * 1024) // T <= 1021 for T in range(48, 401) for k in (T - 1,))
    assert min(48 * q // p for p, q in wave_codec.PITCH_RATIOS.values()) == 33


def test_the_library_builds_in_the_same_window():
    """The committed table equals the fp64 formula (and the function, and the restatement): no libm decides a sample."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(infer.__file__)), "csrc")
    body = "".join(line for line in open(os.path.join(csrc, "psola_window.inc"), encoding="utf-8") if not line.startswith("//"))
    formula = [int(np.rint(32768.0 * (1.0 + np.cos(np.pi * j / 1024.0)) / 2.0)) for j in range(1025)]
    assert [int(v) for v in re.findall(r"-?\d+", body)] == formula == [int(v) for v in wave_codec.psola_window()] == ref.window()
    core = open(os.path.join(csrc, "wave_formant_core.h"), encoding="utf-8").read()
    assert "kFpHop = 120, kFpWin = 480, kFpLagMin = 48, kFpLagMax = 400;" in core and "kFpMinAdvance = 24;" in core and "kFpTable = 1024;" in core


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_psola_equals_the_restatement(kind, n):
    """Every length, every content, all twelve steps: the track, both mark lists and the samples of the plain-integer restatement."""
    x = content(kind, n)
    xs, frames, marks = reference(kind, n)
    lag, voiced = wave_codec.psola_track(x)
    assert list(zip(lag.tolist(), voiced.tolist())) == frames and len(frames) == -(-n // 120)
    a, T, v = wave_codec.psola_marks(x, lag, voiced)
    assert list(zip(a.tolist(), T.tolist(), [bool(f) for f in v])) == marks
    for s in STEPS:
        u, idx = wave_codec.psola_synthesis(a, T, v, n, s)
        assert list(zip(u.tolist(), idx.tolist())) == ref.synthesis_marks(marks, n, s)
        got = wave_codec.psola_pcm16(x, s)
        assert got.dtype == np.int16 and got.tolist() == _ref_output(xs, marks, s), (kind, n, s)


def _ref_output(xs, marks, s):
    n = len(xs)
    M = ref.window()
    num, den = [0] * n, [0] * n
    for u, i in ref.synthesis_marks(marks, n, s):
        a, T, _ = marks[i]
        for k in range(-T, T + 1):
            if 0 <= u + k < n:
                w = M[(abs(k) * ref.TABLE) // T]
                num[u + k] += w * (xs[a + k] if 0 <= a + k < n else 0)
                den[u + k] += w
    return [min(max(xs[j] if den[j] == 0 else (2 * num[j] + den[j]) // (2 * den[j]), -32768), 32767) for j in range(n)]


def test_the_restatement_is_one_function():
    """`reference` caches the restatement's analysis per case; its own `psola` runs the same steps in one go."""
    for kind, n in (("mixed", 1000), ("vowel", 1000), ("square", 480)):
        xs, _, marks = reference(kind, n)
        assert ref.psola(xs, -6) == _ref_output(xs, marks, -6)


def test_the_matrix_reaches_the_rules():
    """The cases are not all trivial: voiced and unvoiced frames, chained and first marks, ties in the peak search, a carried remainder."""
    lag, voiced = wave_codec.psola_track(content("mixed", 30011))
    assert voiced.any() and not voiced.all()
    a, T, v = wave_codec.psola_marks(content("mixed", 30011), lag, voiced)
    runs = np.flatnonzero(np.diff(np.concatenate([[0], v])) == 1)
    assert len(runs) >= 2 and (np.diff(a) >= 24).all() and a[-1] < 30011 <= a[-1] + T[-1]
    lag, voiced = wave_codec.psola_track(content("square", 24000))
    assert voiced[2:-6].all() and set(lag[2:-6].tolist()) == {160}
    a, T, v = wave_codec.psola_marks(content("square", 24000), lag, voiced)
    assert (a[:140] % 160 == 0).all() and v[:140].all()                  # 80 equal samples a plateau: every mark at its first one
    u, _ = wave_codec.psola_synthesis(a, T, v, 24000, 1)
    assert set(np.diff(u[:100]).tolist()) == {151, 152}                  # 160 * 17 = 151 * 18 + 2: the remainder is carried
    assert u[90] - u[0] == 90 * 160 * 17 // 18


def test_length_zero_and_identity_laws():
    for n in LENGTHS:
        for s in (-6, 1, 6):
            for kind in CONTENTS:
                assert len(wave_codec.psola_pcm16(content(kind, n), s)) == n
            assert not wave_codec.psola_pcm16(np.zeros(n, dtype=np.int16), s).any()
    for n in (1, 119, 480, 1000, 24000, 30011):                          # noise at sigma 2000: no voiced frame, the bytes unchanged
        x = noise(n)
        assert not wave_codec.psola_track(x)[1].any()
        for s in (-6, -3, 2, 6):
            assert np.array_equal(wave_codec.psola_pcm16(x, s), x), (n, s)
    with pytest.raises(ValueError, match="non-zero pitch"):
        wave_codec.psola_pcm16(np.zeros(4, dtype=np.int16), 0)
    with pytest.raises(ValueError, match="pitch must be"):
        wave_codec.psola_pcm16(np.zeros(4, dtype=np.int16), 7)
    with pytest.raises(ValueError, match="int16"):
        wave_codec.psola_pcm16(np.zeros(4, dtype=np.float32), 1)


def test_a_requests_bytes_depend_on_that_request_alone():
    """The function takes one wave; what lies around it in a caller's buffer does not enter (a view into a larger array gives the bytes of
    its copy), and the input is not written."""
    x = content("mixed", 30011)
    big = np.concatenate([noise(500, 9000.0, 1), x, vowel(700, 90)])
    view = big[500:500 + len(x)]
    before = big.copy()
    assert np.array_equal(wave_codec.psola_pcm16(view, 5), wave_codec.psola_pcm16(x.copy(), 5)) and np.array_equal(big, before)


# ------------------------------------------------------------------------------------------------ properties, against no code of ours
def _fundamental(y):
    """Hz, from the autocorrelation of samples 6000 .. 15600: the smallest lag in 40 .. 480 whose value is within 5 % of the maximum there
    (a plain argmax picks 2 T now and then), moved up to its local peak, refined by a parabola."""
    s = y[6000:15600].astype(np.float64)
    s = s - s.mean()
    spec = np.fft.rfft(s, 2 * len(s))
    ac = np.fft.irfft(spec * np.conj(spec))[:482]
    lag = 40 + int(np.argmax(ac[40:481] >= 0.95 * ac[40:481].max()))
    while lag < 480 and ac[lag + 1] > ac[lag]:
        lag += 1
    a, b, c = ac[lag - 1], ac[lag], ac[lag + 1]
    return RATE / (lag + 0.5 * (a - c) / (a - 2.0 * b + c))


def _formant(y):
    """Hz of the strongest bin of the mean power spectrum inside 400 .. 1000 Hz: frames of 2048 at hop 512 under a Hann window, FFT 4096."""
    frames = np.lib.stride_tricks.sliding_window_view(y.astype(np.float64), 2048)[::512]
    power = (np.abs(np.fft.rfft(frames * np.hanning(2048), 4096, axis=1)) ** 2).mean(axis=0)
    f = np.arange(len(power)) * RATE / 4096.0
    band = (f >= 400.0) & (f <= 1000.0)
    return float(f[band][np.argmax(power[band])])


@pytest.mark.parametrize("f0", [100, 120, 150])
def test_the_fundamental_moves_and_the_first_formant_stays(f0):
    """2 s vowels with integer periods (240, 200, 160), steps +-3 and +-6.  The fundamental lands within 1e-3 relative of f0 p / q (the
    carried remainder makes the mean spacing exact, so the bound covers the estimator), and the strongest bin in 400 .. 1000 Hz stays within
    one output harmonic spacing of the input's -- the resolution at which harmonics sample an envelope.  At +-6 moving the envelope by p / q
    would miss that bound, so it tells kept from moved; at -6 today's `shift_pcm16` does miss it.

    Measured on the host function: the fundamental is off by at most 1.2e-4 relative (150 Hz, +6); the formant bin moves by at most 99.6 Hz
    against 212.1 (150 Hz, +6), elsewhere by 5.9 to 41.0 Hz against 70.7 to 178.4.  Moved envelopes would be 204 to 310 Hz off; the plain
    shift at -6 is 199 / 211 / 217 Hz off against 70.7 / 84.9 / 106.1."""
    x = vowel(2 * RATE, f0)
    assert abs(_fundamental(x) / f0 - 1.0) < 1e-5
    peak_in = _formant(x)
    for s in (-6, -3, 3, 6):
        p, q = wave_codec.PITCH_RATIOS[s]
        y = wave_codec.psola_pcm16(x, s)
        f_out = f0 * p / q
        got, peak = _fundamental(y), _formant(y)
        print(f"{f0} Hz, step {s}: fundamental off by {abs(got / f_out - 1.0):.2e}, formant bin {peak_in:.1f} -> {peak:.1f} Hz (bound {f_out:.1f})")
        assert abs(got / f_out - 1.0) <= 1e-3, (s, got, f_out)
        assert abs(peak - peak_in) <= f_out, (s, peak, peak_in)
        if abs(s) == 6:
            assert abs(peak_in * p / q - peak_in) > f_out, (s, peak_in)  # the check can tell kept from moved
    plain = _formant(wave_codec.shift_pcm16(x, 1.0, -6))
    assert abs(plain - peak_in) > f0 * 29 / 41, (plain, peak_in)         # today's shift moves the formant with the pitch


# ------------------------------------------------------------------------------------------------ the option
def test_shift_pcm16_takes_the_flag_and_keeps_its_three_argument_form():
    x = content("mixed", 24000)
    assert list(inspect.signature(wave_codec.shift_pcm16).parameters) == ["pcm", "tempo", "pitch", "keep_formants"]
    assert inspect.signature(wave_codec.shift_pcm16).parameters["keep_formants"].default is False
    for tempo, pitch in ((1.0, 4), (1.25, -6), (0.8, 3), (None, 1)):
        hundredths = 100 if tempo is None else round(100 * tempo)
        got = wave_codec.shift_pcm16(x, tempo, pitch, keep_formants=True)
        P, Q = wave_codec.formant_stretch(hundredths)
        assert (P * hundredths, np.gcd(P, Q)) == (Q * 100, 1)
        assert np.array_equal(got, wave_codec.psola_pcm16(wave_codec.wsola_pcm16(x, P, Q), pitch)) and len(got) == -(-len(x) * 100 // hundredths)
        assert len(got) == wave_codec.shifted_length(len(x), (P, Q), 0)
        plain = wave_codec.shift_pcm16(x, tempo, pitch)
        assert np.array_equal(plain, wave_codec.shift_pcm16(x, tempo, pitch, False)) and np.array_equal(plain, wave_codec.shift_pcm16(x, tempo, pitch, keep_formants=None))
        assert not np.array_equal(plain[:1000], got[:1000]) or len(plain) != len(got)
    with pytest.raises(ValueError, match="outside 1/2 to 2"):            # the combined-stretch refusal stays, whatever the flag
        wave_codec.shift_pcm16(x, 0.5, 6, keep_formants=True)


def test_refusals_character_for_character():
    for bad in (1, 0, "true", 1.0, [True]):
        with pytest.raises(ValueError) as e:
            wave_codec.check_keep_formants(bad)
        assert str(e.value) == f"keep_formants must be true or false (got {bad!r})"
        with pytest.raises(ValueError, match="keep_formants must be true or false"):
            wave_codec.shift_pcm16(np.zeros(4, dtype=np.int16), 1.0, 2, keep_formants=bad)
    for pitch in (None, 0):
        with pytest.raises(ValueError) as e:
            wave_codec.shift_pcm16(np.zeros(4, dtype=np.int16), 1.25, pitch, keep_formants=True)
        assert str(e.value) == "keep_formants needs a non-zero pitch"
    assert wave_codec.check_keep_formants(None) is False and wave_codec.check_keep_formants(np.bool_(True), 2) is True
    assert wave_codec.check_keep_formants(False, 0) is False and wave_codec.check_keep_formants(True) is True
    with pytest.raises(ValueError, match="pitch must be"):                # the pitch's own refusal comes first
        wave_codec.shift_pcm16(np.zeros(4, dtype=np.int16), 1.0, 7, keep_formants=True)


def test_the_options_table_and_the_wave_spec():
    assert wave_codec.FORMANT_OPTIONS == infer.FORMANT_OPTIONS == ("keep_formants",)
    assert infer.REQUEST_OPTIONS.index("watermark") == 11 and infer.REQUEST_OPTIONS.index("keep_formants") == 12
    assert infer.REQUEST_OPTIONS[-2:] == infer.PROSODY_OPTIONS == ("tempo", "pitch") and len(infer.REQUEST_OPTIONS) == 15
    assert [f.name for f in dataclasses.fields(infer.WaveSpec)] == list(wave_codec.DELIVERY_OPTIONS) + ["tempo", "pitch", "watermark", "keep_formants"]   # the last field
    assert infer.WaveSpec.of(dict(pitch=2, keep_formants=True)) == infer.WaveSpec(pitch=2, keep_formants=True) != infer.WaveSpec(pitch=2)
    assert infer.WaveSpec.of(dict(pitch=2, keep_formants=False)) == infer.WaveSpec(pitch=2)
    assert "keep_formants" not in serve.EDIT_OPTIONS + serve.EDIT_DELIVERY + serve.EDIT_MARK


def test_check_request_options_and_the_route_models():
    check = serve.check_request_options
    assert check(dict(pitch=-2, keep_formants=True)) == dict(pitch=-2, keep_formants=True)
    assert check(dict(pitch=-2, keep_formants=False)) == dict(pitch=-2) and check(dict(keep_formants=False)) == {} == check(dict(keep_formants=None))
    for bad in (1, "true", 1.0):
        with pytest.raises(ValueError) as e:
            check(dict(pitch=2, keep_formants=bad))
        assert str(e.value) == f"keep_formants must be true or false (got {bad!r})"
    for opts in (dict(keep_formants=True), dict(keep_formants=True, pitch=0), dict(keep_formants=True, tempo=1.25)):
        with pytest.raises(ValueError) as e:
            check(opts)
        assert str(e.value) == "keep_formants needs a non-zero pitch"
    with pytest.raises(ValueError, match="outside 1/2 to 2"):
        check(dict(tempo=0.5, pitch=3, keep_formants=True))
    with pytest.raises(ValueError, match="unknown option"):                # not on the edit route: its options are pinned
        check(dict(keep_formants=True), allowed=tuple(dict.fromkeys(serve.EDIT_OPTIONS + serve.EDIT_DELIVERY + serve.EDIT_MARK)))
    assert serve.stream_refusal(dict(pitch=2, keep_formants=True)) == serve.STREAM_PROSODY
    models = serve.request_models()
    for model in (models.KannadaSynthesizeRequest, models.SynthesizeRequest, models.CloneRequest, models.ScriptRequest):
        assert "keep_formants" in model.model_fields and set(infer.REQUEST_OPTIONS) <= set(model.model_fields), model
    assert "keep_formants" not in models.EditRequest.model_fields
    assert "keep_formants" not in inspect.signature(serve.TTSManager.edit).parameters


def test_finish_pcm16_is_the_composition_with_the_new_step():
    """After silence removal, before watermark, loudness and rate / encoding."""
    speech = content("mixed", RATE)
    pause = np.concatenate([speech, np.zeros(int(2.5 * RATE), dtype=np.int16), vowel(RATE, 120)])
    cut = infer.remove_silence_pcm(pause, RATE)
    assert len(cut) < len(pause)
    option_sets = [dict(pitch=-2), dict(tempo=0.8, pitch=3, remove_silence=True), dict(pitch=5, loudness=-20.0),
                   dict(pitch=1, sample_rate=8000, encoding="mulaw"), dict(tempo=1.1, pitch=-6, encoding="flac", flac_level=1, loudness=-23.0, remove_silence=True)]
    for opts in option_sets:
        for key in (None, 99):
            spec = infer.WaveSpec.of(opts)
            x = cut if spec.remove_silence else pause
            y = wave_codec.mark_pcm16(wave_codec.shift_pcm16(x, spec.tempo, spec.pitch, keep_formants=True), key)
            want = infer.deliver_pcm16(infer.normalise_loudness_pcm16(y, spec.loudness), *spec.format, flac_level=spec.flac_level if spec.flac else None)
            got = infer.finish_pcm16(pause, dataclasses.replace(spec, watermark=key, keep_formants=True))
            assert got.dtype == want.dtype and np.array_equal(got, want), opts
            today = infer.finish_pcm16(pause, dataclasses.replace(spec, watermark=key))
            assert np.array_equal(today, infer.finish_pcm16(pause, dataclasses.replace(spec, watermark=key, keep_formants=False))) and not (len(today) == len(got) and np.array_equal(today, got))


def test_finish_requests_takes_the_option_per_request():
    fade = infer.cross_fade_duration
    f = lambda x: x.astype(np.float32) / 32768.0   # noqa: E731
    reqs = [[f(vowel(20000, 110))], [f(vowel(15000, 150)), f(content("mixed", 14000))], [f(vowel(9000, 200, 140))]]
    texts, flags = ["x"] * 3, [False] * 3
    plain = infer.finish_requests(reqs, texts, fade, flags, want="pcm16")
    got = infer.finish_requests(reqs, texts, fade, flags, tempo=[1.25, None, 0.8], pitch=[4, 2, -1], keep_formants=[True, False, True])
    for g, x, (t, s, k) in zip(got, plain, ((1.25, 4, True), (None, 2, False), (0.8, -1, True))):
        assert g.dtype == np.int16 and np.array_equal(g, wave_codec.shift_pcm16(x, t, s, keep_formants=k))
    one = infer.finish_requests(reqs, texts, fade, flags, pitch=3, keep_formants=True)                 # one value for all
    assert all(np.array_equal(g, wave_codec.shift_pcm16(x, None, 3, keep_formants=True)) for g, x in zip(one, plain))
    today = infer.finish_requests(reqs, texts, fade, flags, pitch=3)
    assert all(np.array_equal(a, b) for a, b in zip(today, infer.finish_requests(reqs, texts, fade, flags, pitch=3, keep_formants=False)))
    waves = infer.SegmentedWaves([reqs[1], reqs[2]], RATE // 2)                       # a script is shifted as one joined wave
    joined = infer.quantise_pcm16(infer.join_segments([reqs[1], reqs[2]], fade, RATE // 2))
    assert np.array_equal(infer.finish_requests([waves], ["x"], fade, [False], tempo=0.9, pitch=1, keep_formants=True)[0],
                          wave_codec.shift_pcm16(joined, 0.9, 1, keep_formants=True))
    with pytest.raises(ValueError) as e:
        infer.finish_requests(reqs, texts, fade, flags, keep_formants=True)
    assert str(e.value) == "keep_formants needs a non-zero pitch"
    with pytest.raises(ValueError, match="keep_formants must be true or false"):
        infer.finish_requests(reqs, texts, fade, flags, pitch=2, keep_formants=1)
    with pytest.raises(ValueError) as e:
        infer.finish_requests([reqs[0]], [["head"]], fade, pitch=2, keep_formants=True)    # a list of chunk texts: the pitch's message
    assert str(e.value) == infer.WHOLE_WAVE_PROSODY


def test_the_planner_carries_the_flag_beside_the_spec(tmp_path):
    voice = infer.PreparedVoice(_voice(tmp_path))
    plan = lambda text, opts: infer.plan_request((voice, "reference words", text, opts), DEFAULTS, target_rms=0.1, fix_duration=None, device=None,   # noqa: E731
                                                 tokenizer=infer.text_to_tokens)
    got = plan("some text.", dict(pitch=1, keep_formants=True))
    assert dataclasses.replace(got.spec, keep_formants=False) == infer.WaveSpec(pitch=1) and got.spec.keep_formants is True   # the flag leaves every other field alone
    assert plan("some text.", dict(pitch=1)).spec.keep_formants is False and plan("some text.", {}).spec.keep_formants is False
    with pytest.raises(ValueError) as e:
        plan("text.", dict(keep_formants=True))
    assert str(e.value) == "keep_formants needs a non-zero pitch"
    with pytest.raises(ValueError, match="keep_formants must be true or false"):
        plan("text.", dict(pitch=2, keep_formants="yes"))
    for text in (["one chunk.", "another chunk."], ("one chunk.",)):
        with pytest.raises(ValueError) as e:
            plan(text, dict(pitch=-3, keep_formants=True))
        assert str(e.value) == infer.WHOLE_WAVE_PROSODY


def test_manager_and_speech_routes(client, tmp_path):
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    pcm = infer.quantise_pcm16(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text))
    want = wave_codec.shift_pcm16(pcm, 1.25, -2, keep_formants=True)
    got = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, tempo=1.25, pitch=-2, keep_formants=True)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, pitch=-2, keep_formants=False), wave_codec.shift_pcm16(pcm, None, -2))
    raw = open(_voice(tmp_path), "rb").read()
    clip_pcm = infer.quantise_pcm16(mgr.synthesize_clip(TEXT, raw, "reference words"))
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words", pitch=3, keep_formants=True), wave_codec.shift_pcm16(clip_pcm, None, 3, keep_formants=True))
    with pytest.raises(ValueError) as e:
        mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, keep_formants=True)
    assert str(e.value) == "keep_formants needs a non-zero pitch"
    for stream in (mgr.synthesize_stream, lambda *a, **kw: mgr.synthesize_clip_stream(TEXT, raw, "reference words", **kw)):
        with pytest.raises(ValueError) as e:
            stream(TEXT, voice.audio_path, voice.ref_text, pitch=1, keep_formants=True)
        assert str(e.value) == serve.STREAM_PROSODY
    body = dict(text=TEXT, tempo=1.25, pitch=-2, keep_formants=True)
    clone = dict(body, ref_audio=base64.b64encode(raw).decode(), ref_text="reference words")
    for route, extra in (("/v1/audio/speech", body), ("/v1/audio/speech/voice", dict(body, ref_audio_name="KAN_F (Happy)")), ("/v1/audio/speech/clone", clone)):
        r = c.post(route, json=dict(extra, response_format="pcm"))
        assert r.status_code == 200, (route, r.text)
        assert r.content == (want if "clone" not in route else wave_codec.shift_pcm16(clip_pcm, 1.25, -2, keep_formants=True)).tobytes(), route
        r = c.post(route, json=dict(extra, stream=True))
        assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_PROSODY, route
        for bad in (1, "true", 0.5):
            r = c.post(route, json=dict(extra, keep_formants=bad))
            assert r.status_code == 400 and r.json()["detail"] == f"keep_formants must be true or false (got {bad!r})", (route, bad)
        r = c.post(route, json=dict(extra, pitch=0))
        assert r.status_code == 400 and r.json()["detail"] == "keep_formants needs a non-zero pitch", route
        r = c.post(route, json={k: v for k, v in extra.items() if k != "pitch"})
        assert r.status_code == 400 and r.json()["detail"] == "keep_formants needs a non-zero pitch", route
    r = c.post("/v1/audio/speech", json=dict(body, sample_rate=8000, encoding="mulaw", loudness=-20.0, response_format="pcm"))
    assert r.status_code == 200 and r.content == infer.deliver_pcm16(infer.normalise_loudness_pcm16(want, -20.0), 8000, "mulaw").tobytes()
    r = c.post("/v1/audio/speech", json=dict(text=TEXT, keep_formants=False, stream=True))                  # neutral: streams as today
    assert r.status_code == 200


def test_script_route_and_method(script_client):
    c, mgr, path = script_client
    mgr.load(NoiseModel(), Vocoder())
    voices = dict(main=dict(ref_audio_path=path, ref_text=RA), town=dict(ref_audio=_wav(B), ref_text=RB))
    pcm = infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4))
    want = wave_codec.shift_pcm16(pcm, 0.9, 2, keep_formants=True)
    got = mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4, tempo=0.9, pitch=2, keep_formants=True)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    with pytest.raises(ValueError) as e:
        mgr.synthesize_script_stream(SCRIPT, voices, pitch=2, keep_formants=True)
    assert str(e.value) == serve.STREAM_PROSODY
    town = dict(ref_audio=base64.b64encode(_wav(B)).decode(), ref_text=RB)
    body = dict(text=SCRIPT, voices=dict(main=dict(ref_audio_name="KAN_F (Happy)"), town=town), seed=4, gap=0.5, tempo=0.9, pitch=2, keep_formants=True)
    r = c.post("/v1/audio/speech/script", json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
    calls = len(mgr.model_obj.calls)
    r = c.post("/v1/audio/speech/script", json=dict(body, stream=True))
    assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_PROSODY
    r = c.post("/v1/audio/speech/script", json=dict(body, pitch=0))
    assert r.status_code == 400 and r.json()["detail"] == "keep_formants needs a non-zero pitch"
    r = c.post("/v1/audio/speech/script", json=dict(body, keep_formants="yes"))
    assert r.status_code == 400 and "keep_formants must be true or false" in r.json()["detail"]
    assert len(mgr.model_obj.calls) == calls                                            # none reached the sampler


def test_span_scheduler_carries_the_flag():
    """`SpanScheduler.admit` plans the flag into the spec and its tickets hand it to the finishing chain: with the same seed the kept
    request is `shift_pcm16(..., keep_formants=True)` of the request without options, and the plain pitch is today's."""
    from test_spans import FakeModel, FakeVocoder, _request as span_request, _voice as span_voice
    voice = span_voice()
    sched = infer.SpanScheduler(FakeModel(), FakeVocoder(), span_steps=3, nfe_step=4)
    text = "A sentence for the scheduler."
    tickets = [sched.admit(span_request(voice, text, seed=3, **opts)) for opts in ({}, dict(pitch=3), dict(pitch=3, keep_formants=True), dict(tempo=0.9, pitch=-2, keep_formants=True))]
    assert [t.spec.keep_formants for t in tickets] == [False, False, True, True]
    while sched.busy:
        sched.step()
    plain = infer.quantise_pcm16(tickets[0].result)
    assert np.array_equal(tickets[1].result, wave_codec.shift_pcm16(plain, None, 3))
    assert np.array_equal(tickets[2].result, wave_codec.shift_pcm16(plain, None, 3, keep_formants=True)) and len(tickets[2].result) == len(plain)
    assert np.array_equal(tickets[3].result, wave_codec.shift_pcm16(plain, 0.9, -2, keep_formants=True))
    with pytest.raises(ValueError, match="keep_formants needs a non-zero pitch"):
        sched.admit(span_request(voice, text, keep_formants=True))
