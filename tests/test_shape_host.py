"""CPU: `pitch` as `{"semitones": s, "formant": f}` on the host: `wave_codec.psola_shape_pcm16` against tests/shape_ref.py, its laws, the
option's normal form and refusals, and its place in the finishing order."""
import numpy as np
import pytest
import shape_ref
from tts_indic_server_f5_amd import infer, serve, wave_codec

from test_formant_host import LENGTHS, RATE, _formant, _fundamental, content, reference, vowel
from test_wave_encode_host import TEXT, client  # noqa: F401  (the stand-in manager behind a TestClient)

KINDS = ("zeros", "noise", "vowel", "mixed")
MOVES = [(0, 1), (0, -6), (0, 6), (3, -3), (-2, 4), (6, 0)]
Tag = wave_codec.PitchTag


def _case(kind, n):
    """(x, its samples as a list, its analysis marks); "inside" begins in a voiced stretch: its first grain interpolates from in front of the wave."""
    if kind != "inside":
        return (content(kind, n),) + reference(kind, n)[::2]
    x = vowel(30011, 130)[6000:6000 + n]
    return x, x.tolist(), shape_ref.ref.analysis_marks(x.tolist(), shape_ref.ref.track(x.tolist()))


@pytest.mark.parametrize("kind,n", [(k, n) for n in LENGTHS for k in KINDS] + [("inside", 3000)])
def test_shape_equals_the_restatement_and_keeps_its_laws(kind, n):
    x, xs, marks = _case(kind, n)
    for s, f in MOVES:
        got = wave_codec.psola_shape_pcm16(x, s, f)
        assert got.dtype == np.int16 and len(got) == n and got.tolist() == shape_ref.shape(xs, marks, s, f), (kind, n, s, f)
        assert f or np.array_equal(got, wave_codec.psola_pcm16(x, s))                      # formant = 0 is the pitch shift that keeps them
        assert any(m[2] for m in marks) or np.array_equal(got, x)                          # zeros stay zeros; noise comes back byte for byte
    big = np.concatenate([vowel(700, 90), x, content("noise", 500)])                       # nothing but the request's own samples enters
    assert np.array_equal(wave_codec.psola_shape_pcm16(big[700:700 + n], -2, 4), wave_codec.psola_shape_pcm16(x, -2, 4))


def test_the_option_normalises_and_refuses():
    of = lambda p, **kw: infer.WaveSpec.of(dict(pitch=p, **kw))   # noqa: E731
    assert of({"semitones": 2}) == of({"semitones": 2, "formant": 0}) == of(2) == infer.WaveSpec(pitch=2)
    assert of({"formant": 4}).pitch == Tag(0, 4) == wave_codec.check_pitch(Tag(0, 4)) and of({"semitones": 6, "formant": 3}, tempo=0.5).stretch == (2, 1)
    assert of({"semitones": 4, "formant": -2}, keep_formants=True) == of({"semitones": 4, "formant": -2}) == infer.WaveSpec(pitch=Tag(4, -2))
    assert serve.check_request_options(dict(pitch={"semitones": 1, "formant": 0})) == dict(pitch=1)
    assert serve.check_request_options(dict(pitch={"formant": -3}, tempo=1.25)) == dict(pitch=Tag(0, -3), tempo=1.25)
    assert serve.stream_refusal(dict(pitch=Tag(0, 2))) == serve.STREAM_PROSODY
    refusals = [({}, "pitch as a mapping needs semitones or formant (got {})"),
                ({"formant": 2, "cents": 5}, "pitch has an unknown entry 'cents': a pitch with a formant shift is {\"semitones\": s, \"formant\": f}"),
                ({"formant": 2.0}, "pitch formant must be a whole number of semitones from -6 to 6 (got 2.0)"),
                ({"semitones": True}, "pitch semitones must be a whole number of semitones from -6 to 6 (got True)"),
                ({"formant": 7}, "pitch formant must be a whole number of semitones from -6 to 6 (got 7)"),
                ({"semitones": -3, "formant": 4}, "pitch formant 4 beside semitones -3 is 7 semitones apart: at most 6, or the grains leave gaps")]
    for bad, text in refusals:
        for call in (wave_codec.check_pitch, of, lambda p: serve.check_request_options(dict(pitch=p))):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == text
    with pytest.raises(ValueError) as e:                                                   # a list of chunk texts: the pitch's own message
        infer.finish_requests([[np.zeros(9000, dtype=np.float32)]], [["head"]], pitch={"formant": 2})
    assert str(e.value) == infer.WHOLE_WAVE_PROSODY


def test_finish_requests_and_a_route_compose_in_the_written_order(client):  # noqa: F811
    """Tempo (WSOLA by the tempo alone), the shaped PSOLA, the watermark, then loudness."""
    reqs = [[vowel(20000, 110).astype(np.float32) / 32768.0], [content("mixed", 14000).astype(np.float32) / 32768.0]]
    plain = infer.finish_requests(reqs, ["x"] * 2, want="pcm16")
    got = infer.finish_requests(reqs, ["x"] * 2, tempo=[1.25, None], pitch=[{"semitones": 4, "formant": -2}, 3], watermark=99, loudness=-20.0)
    want = [wave_codec.psola_shape_pcm16(wave_codec.wsola_pcm16(plain[0], 4, 5), 4, -2), wave_codec.shift_pcm16(plain[1], None, 3)]
    assert all(np.array_equal(g, infer.normalise_loudness_pcm16(wave_codec.mark_pcm16(w, 99), -20.0)) for g, w in zip(got, want))
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    pcm = infer.quantise_pcm16(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text))
    r = c.post("/v1/audio/speech", json=dict(text=TEXT, tempo=0.8, pitch={"semitones": 0, "formant": 4}, response_format="pcm"))
    assert r.status_code == 200 and r.content == wave_codec.shift_pcm16(pcm, 0.8, Tag(0, 4)).tobytes()
    r = c.post("/v1/audio/speech", json=dict(text=TEXT, pitch={"formant": 9}))
    assert r.status_code == 400 and r.json()["detail"] == "pitch formant must be a whole number of semitones from -6 to 6 (got 9)"


@pytest.mark.parametrize("f0", [100, 120, 150])
def test_the_first_formant_moves_and_the_fundamental_stays(f0):
    """2 s vowels, formant steps +-3 and +-6, no pitch, with the margins tests/test_formant_host.py uses for the opposite claim: the
    fundamental within 1e-3 relative of f0, the strongest bin of the band (400 .. 1000 Hz, widened by P / Q) within one harmonic spacing,
    f0, of peak_in P / Q; at +-6 the unshifted place misses that bound.  Measured on the host function: the fundamental is off by at most
    1.25e-4 (100 Hz, -6); the bin lands 4.9 to 67.2 Hz from peak_in P / Q -- worst 67.2 against 150 (150 Hz, -6) and 58.0 against 120
    (120 Hz, +6) -- while the unshifted place is 204 to 310 Hz away at +-6.  Linear interpolation misses no margin."""
    x = vowel(2 * RATE, f0)
    for f in (-6, -3, 3, 6):
        y, want = wave_codec.psola_shape_pcm16(x, 0, f), _formant(x) * wave_codec.PITCH_RATIOS[f][0] / wave_codec.PITCH_RATIOS[f][1]
        frames = np.lib.stride_tricks.sliding_window_view(y.astype(np.float64), 2048)[::512]    # `_formant`, its band widened by the ratio
        power = (np.abs(np.fft.rfft(frames * np.hanning(2048), 4096, axis=1)) ** 2).mean(axis=0)
        lo, hi = int(np.ceil(min(400, 400 * want / _formant(x)) * 4096 / RATE)), int(np.floor(max(1000, 1000 * want / _formant(x)) * 4096 / RATE))
        peak = (lo + int(np.argmax(power[lo:hi + 1]))) * RATE / 4096.0
        assert abs(_fundamental(y) / f0 - 1.0) <= 1e-3 and abs(peak - want) <= f0, (f, peak, want)
        assert abs(f) != 6 or abs(_formant(x) - want) > f0                                  # the check can tell moved from kept
