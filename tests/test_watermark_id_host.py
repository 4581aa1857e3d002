"""The watermark's trace ids on the host (CPU): `wave_codec.watermark_subkey`, `mark_pcm16` of a `WatermarkTag` and `read_watermark` against
their known answers, their plain restatement (tests/watermark_id_ref.py) and their laws; the detection figures on the suite's synthetic
speech-like hosts (tests/watermark_ref.py `host`, peak 12 000, key 1 -- not real speech); the tag through the planner, `finish_requests`, the
manager and the routes over stand-in models.

The mark is compared as bytes.  The read's bounds are the issue's: on clean 1 s hosts, seeds 0 .. 11, every id reads right; id_z >= 6.5 on
3 s hosts clean and after each delivery step; every z_d < 5.5 and no id on key-only, unmarked and other-key clips (the threshold is 6);
z >= 10 for the key of a tagged 1 s clip; definition against restatement: the same ids, |dz| <= 1e-9 (both fp64: FFT correlations against
direct sums).  The twelve ids are the first twelve draws of `numpy.random.default_rng(0)`; the smallest id_z of twelve clips moves by about
+- 0.6 with the ids drawn (measured on the host over seven id streams: 3 s cut by 7001 samples 6.40 .. 8.01, 1 s clean 6.11 .. 6.95)."""
import base64
import dataclasses

import numpy as np
import pytest
import torch

import watermark_id_ref as idref
import watermark_ref as ref
from tts_indic_server_f5_amd import infer, serve, wave_codec
from tts_indic_server_f5_amd.wave_codec import WatermarkTag

from test_script_host import RA, RB, SCRIPT, NoiseModel, Vocoder, _wav, B  # noqa: E402
from test_script_host import client as script_client  # noqa: E402,F401  (a manager without a model behind a TestClient)
from test_watermark_host import DEFAULTS, _content, _to_24k, _wav24  # noqa: E402
from test_wave_encode_host import TEXT, _voice, client  # noqa: E402,F401  (the stand-in manager behind a TestClient)

RATE = 24000
KEY = 1
MIXED = 0x2A5F3C91                                                                     # symbols 145, 975, 677
IDS = [int(v) for v in np.random.default_rng(0).integers(0, 2 ** 30, 12)]              # one per seed
MARK_LENGTHS = (1, 239, 240, 241, 481, 7680, 16385, 40000)


def _read(wave, key=KEY):
    return wave_codec.read_watermark(wave, [key])[0]


def _symbols(clip, key=KEY):
    """[(s_d, z_d)] of a clip for a key, from the definition's pieces."""
    FZ = np.conj(np.fft.rfft(wave_codec.watermark_fold(clip)))
    corr = lambda k: np.fft.irfft(FZ * np.fft.rfft(wave_codec.watermark_carrier(k).astype(np.float64)), n=wave_codec.WATERMARK_PERIOD)   # noqa: E731
    offset = wave_codec.watermark_score(corr(key), key).offset
    return [wave_codec.watermark_symbol(corr(sub), offset) for sub in wave_codec.watermark_subkeys(key)]


@pytest.fixture(scope="module")
def tagged3():
    """Seeds 0 .. 11: the 3 s host marked with key 1 and the seed's id (read-only)."""
    out = []
    for seed in range(12):
        y = wave_codec.mark_pcm16(ref.host(3 * RATE, seed), WatermarkTag(KEY, IDS[seed]))
        y.setflags(write=False)
        out.append(y)
    return out


# ------------------------------------------------------------------------------------------------ constants and known answers
def test_constants_and_known_answers():
    assert (wave_codec.WATERMARK_ID_BITS, wave_codec.WATERMARK_ID_SYMBOLS, wave_codec.WATERMARK_ID_STEP) == (30, 3, 16)
    assert wave_codec.WATERMARK_ID_MAX == 2 ** 30 - 1 and wave_codec.WATERMARK_ID_THRESHOLD == 6.0
    assert (idref.ID_BITS, idref.SYMBOLS, idref.STEP, idref.ID_MAX, idref.ID_THRESHOLD) == (30, 3, 16, 2 ** 30 - 1, 6.0)
    assert [wave_codec.watermark_subkey(1, d) for d in range(3)] == [160832003273966, 194807364317806, 17338898203305]
    for key in (1, 0xDEADBEEF, 2 ** 48 - 1):
        subs = [wave_codec.watermark_subkey(key, d) for d in range(3)]
        assert subs == [idref.subkey(key, d) for d in range(3)] == wave_codec.watermark_subkeys(key)
        assert all(1 <= s <= wave_codec.WATERMARK_KEY_MAX and wave_codec.check_watermark(s) == s for s in subs) and len({key, *subs}) == 4
    for bad in (3, -1, True, 1.0):
        with pytest.raises(ValueError, match="watermark_subkey"):
            wave_codec.watermark_subkey(1, bad)
    with pytest.raises(ValueError, match="integer key"):
        wave_codec.watermark_subkey(0, 0)
    assert wave_codec.watermark_id_symbols(MIXED) == [145, 975, 677] == idref.symbols(MIXED)
    assert wave_codec.watermark_id_symbols(2 ** 30 - 1) == [1023] * 3 and wave_codec.watermark_id_symbols(1024) == [0, 1, 0]
    assert infer.WatermarkTag is WatermarkTag and infer.read_watermark is wave_codec.read_watermark and infer.WATERMARK_ID_MAX == 2 ** 30 - 1


def test_check_watermark_on_tags_and_bad_values():
    check = wave_codec.check_watermark
    assert check(None) is None and check(77) == 77 and type(check(np.int64(77))) is int             # as pinned
    for bad in (True, 1.5, "7", 0, 2 ** 48, [1], (1, 2)):
        with pytest.raises(ValueError, match="watermark must be an integer key from 1 to 2\\^48 - 1"):
            check(bad)
    tag = check({"key": 5, "id": 9})
    assert tag == WatermarkTag(5, 9) and isinstance(tag, WatermarkTag) and (tag.key, tag.id) == (5, 9)
    assert check(tag) == tag and check({"key": np.int64(5), "id": np.int32(0)}) == WatermarkTag(5, 0)
    assert check({"key": 5}) == 5 and check({"key": 5, "id": None}) == 5
    assert check({"id": 9}, 5) == WatermarkTag(5, 9) == check({"id": 9}, WatermarkTag(5, 3)) and check({"key": 6, "id": 9}, 5) == WatermarkTag(6, 9)
    assert check({"id": 2 ** 30 - 1, "key": 2 ** 48 - 1}) == WatermarkTag(2 ** 48 - 1, 2 ** 30 - 1)
    for bad in (True, 1.0, "3", -1, 2 ** 30):
        with pytest.raises(ValueError) as e:
            check({"key": 5, "id": bad})
        assert str(e.value) == f"watermark id must be an integer from 0 to 2^30 - 1 (got {bad!r})"
    for bad in (True, 1.5, "7", 0, 2 ** 48):
        with pytest.raises(ValueError, match="watermark must be an integer key"):
            check({"key": bad, "id": 1})
    with pytest.raises(ValueError, match="unknown entry 'tenant'"):
        check({"key": 5, "id": 1, "tenant": 2})
    for bad in ({"id": 9}, {}):
        with pytest.raises(ValueError, match="id without a key"):
            check(bad)
    with pytest.raises(ValueError, match="integer key"):
        wave_codec.check_watermark_keys([{"key": 5, "id": 1}])                                      # a clip is scored against keys, not tags
    assert wave_codec.watermark_key(None) is None and wave_codec.watermark_key(7) == 7 and wave_codec.watermark_key(WatermarkTag(7, 1)) == 7


# ------------------------------------------------------------------------------------------------ the mark
@pytest.mark.parametrize("n", MARK_LENGTHS)
def test_mark_equals_the_restatement(n):
    for kind, key in (("speech", 1), ("full", 0xDEADBEEF), ("noise", 1)):
        x = _content(kind, n)
        for tag in (0, 2 ** 30 - 1, MIXED):
            y = wave_codec.mark_pcm16(x, WatermarkTag(key, tag))
            assert y.dtype == np.int16 and len(y) == n and np.array_equal(y, idref.mark(x, key, tag)), (kind, n, tag)
        assert np.array_equal(idref.mark(x, key), ref.mark(x, key))                                  # the restatements agree on a key alone


def test_combined_carrier():
    for tag in (0, MIXED):
        C = wave_codec.watermark_tag_carrier(WatermarkTag(KEY, tag))
        assert C.dtype == np.int64 and C.tolist() == idref.combined(KEY, tag) and np.abs(C).max() <= 5 * 4336
    assert np.array_equal(wave_codec.watermark_tag_carrier(KEY), 2 * wave_codec.watermark_carrier(KEY).astype(np.int64))
    assert not np.array_equal(wave_codec.watermark_tag_carrier(WatermarkTag(KEY, 0)), wave_codec.watermark_tag_carrier(WatermarkTag(KEY, 1)))


def test_mark_laws():
    x = ref.host(50000, 3)
    for wave in (x, _content("full", 40000), _content("noise", 16385), x[:1]):
        for key in (1, 0xDEADBEEF):
            want = wave_codec.mark_pcm16(wave, key)
            assert np.array_equal(wave_codec.mark_pcm16(wave, {"key": key}), want)                   # a key-only tag: `mark_pcm16(pcm, key)`
    zeros = np.zeros(50000, dtype=np.int16)
    assert not wave_codec.mark_pcm16(zeros, WatermarkTag(1, MIXED)).any()                            # zeros stay zeros
    assert len(wave_codec.mark_pcm16(np.zeros(0, dtype=np.int16), WatermarkTag(1, 5))) == 0
    y = wave_codec.mark_pcm16(x, WatermarkTag(1, MIXED))
    assert len(y) == len(x) and not np.array_equal(y, wave_codec.mark_pcm16(x, 1)) and not np.array_equal(y, wave_codec.mark_pcm16(x, WatermarkTag(1, MIXED + 1)))
    assert np.array_equal(y, wave_codec.mark_pcm16(x, {"key": 1, "id": MIXED}))
    # |C| <= 5 * 4336 and E <= 240 * 32768 = 0.9375 * 2^23: |E C| / 2^24 <= 21680 * 0.9375 / 2 = 10162.5, so |y - x| <= 10163
    assert wave_codec.WATERMARK_ID_DELTA_MAX == 10163 == -((-240 * 32768 * 5 * 4336) >> 24)
    for wave in (x, _content("full", 40000), np.full(40000, 32767, dtype=np.int16), np.full(40000, -32768, dtype=np.int16)):
        for tag in (WatermarkTag(1, 0), WatermarkTag(1, MIXED), WatermarkTag(0xDEADBEEF, 2 ** 30 - 1)):
            assert np.abs(wave_codec.mark_pcm16(wave, tag).astype(np.int64) - wave).max() <= wave_codec.WATERMARK_ID_DELTA_MAX
    # locality: output block b depends on input blocks b - 1 .. b + 1 only
    rng = np.random.default_rng(0)
    for b in (0, 7, 100, 207):
        x2 = x.copy()
        x2[240 * b:240 * (b + 1)] = rng.integers(-20000, 20000, len(x2[240 * b:240 * (b + 1)]))
        y2 = wave_codec.mark_pcm16(x2, WatermarkTag(1, MIXED))
        lo, hi = 240 * max(b - 1, 0), 240 * (b + 2)
        assert np.array_equal(y2[:lo], y[:lo]) and np.array_equal(y2[hi:], y[hi:]) and not np.array_equal(y2[lo:hi], y[lo:hi])
    quiet = x.copy()
    quiet[10000:20000] = 0
    yq = wave_codec.mark_pcm16(quiet, WatermarkTag(1, MIXED))
    assert not yq[240 * 43:240 * 82].any() and yq[:9000].any()


# ------------------------------------------------------------------------------------------------ the read
def test_read_equals_the_restatement():
    clips = [wave_codec.mark_pcm16(ref.host(3 * RATE, 1), WatermarkTag(1, MIXED)), ref.host(16385, 2, noisy=True),
             wave_codec.mark_pcm16(ref.host(2 * RATE, 3), WatermarkTag(3, 1023))[5000:].astype(np.float32) / 32768.0]
    for clip in clips:
        for g, (key, z, offset, detected, tag, id_z) in zip(wave_codec.read_watermark(clip, [1, 3]), idref.read(clip, [1, 3])):
            assert g.key == key and abs(g.z - z) <= 1e-9 and g.detected == detected and g.id == tag and abs(g.id_z - id_z) <= 1e-9, (g, z, tag, id_z)
            if detected:
                assert g.offset == offset
    assert [g.id for g in wave_codec.read_watermark(clips[0], [1, 3])] == [MIXED, None]
    got = wave_codec.read_watermark(clips[2], [1, 3])
    assert [g.id for g in got] == [None, 1023] and got[1].offset == 5000
    for clip in clips:                                                                               # the key's part is `detect_watermark`'s
        assert [tuple(g)[:4] for g in wave_codec.read_watermark(clip, [1, 3])] == [tuple(s) for s in wave_codec.detect_watermark(clip, [1, 3])]


def test_read_input_rules():
    y = wave_codec.mark_pcm16(ref.host(RATE, 0), WatermarkTag(1, 5))
    assert wave_codec.read_watermark(y[:11999], [1, 2]) == [wave_codec.WatermarkRead(1, 0.0, 0, False, None, 0.0), wave_codec.WatermarkRead(2, 0.0, 0, False, None, 0.0)]
    assert [tuple(r) for r in wave_codec.read_watermark(y[:11999], [1, 2])] == idref.read(y[:11999], [1, 2])
    assert _read(np.zeros(RATE, dtype=np.int16)) == wave_codec.WatermarkRead(1, 0.0, 0, False, None, 0.0)   # sigma = 0
    assert _read(y) == _read(y.astype(np.float64) / 32768.0) == _read(torch.from_numpy(y))
    with pytest.raises(ValueError, match="watermark keys"):
        wave_codec.read_watermark(y, [])
    with pytest.raises(ValueError, match="not finite"):
        wave_codec.read_watermark(np.array([np.nan] * 20000), [1])
    rule = wave_codec.watermark_read
    score = wave_codec.WatermarkScore(1, 8.0, 3, True)
    assert rule(score, [(1, 6.0), (2, 7.0), (3, 9.0)]) == wave_codec.WatermarkRead(1, 8.0, 3, True, 1 | 2 << 10 | 3 << 20, 6.0)
    assert rule(score, [(1, 5.99), (2, 7.0), (3, 9.0)]).id is None and rule(wave_codec.WatermarkScore(1, 6.9, 3, False), [(1, 9.0)] * 3).id is None
    r = np.zeros(wave_codec.WATERMARK_PERIOD)
    r[[100, 100 - 16 * 5, (100 - 16 * 7) % 16384]] = 1.0
    assert wave_codec.watermark_symbol(r, 100)[0] == 0                                               # ties go to the smaller symbol
    r[100] = 0.5
    assert wave_codec.watermark_symbol(r, 100)[0] == 5


def test_ids_on_clean_one_second_hosts():
    """Seeds 0 .. 11, key 1, 1 s at peak 12 000: every id read right and not null; the key still scores z >= 10."""
    for seed in range(12):
        y = wave_codec.mark_pcm16(ref.host(RATE, seed), WatermarkTag(KEY, IDS[seed]))
        got = _read(y)
        assert got.id == IDS[seed] and got.id_z >= wave_codec.WATERMARK_ID_THRESHOLD and got.offset == 0, (seed, got)
        score = wave_codec.detect_watermark(y, [KEY])[0]
        assert score.z >= 10.0 and score.detected and tuple(got)[:4] == tuple(score), (seed, score)


def test_ids_on_three_second_hosts_and_through_the_delivery_chain(tagged3):
    steps = (("clean", lambda y: y),
             ("mu-law", lambda y: infer.decode_g711(infer.encode_g711(y, "mulaw"), "mulaw")),
             ("8 kHz A-law and back", lambda y: _to_24k(infer.decode_g711(infer.encode_g711(infer.resample_pcm16(y, 8000), "alaw"), "alaw"))),
             ("normalise_loudness_pcm16(-30)", lambda y: infer.normalise_loudness_pcm16(y, -30.0)),
             ("first 7001 samples cut off", lambda y: y[7001:]))
    for name, step in steps:
        for seed, y in enumerate(tagged3):
            got = _read(step(y))
            print(f"{name}: seed {seed} id_z {got.id_z:.2f} z {got.z:.2f}")
            assert got.id == IDS[seed] and got.id_z >= 6.5, (name, seed, got)
            if name.startswith("first"):
                assert got.offset == 7001


def test_edge_ids():
    x = ref.host(3 * RATE, 0)
    for tag in (0, 2 ** 30 - 1, 1023, 1024, 2 ** 20):
        assert _read(wave_codec.mark_pcm16(x, WatermarkTag(KEY, tag))).id == tag


def test_no_false_symbols():
    """Key-only clips of the same key, unmarked clips and clips tagged under another key, 1 s and 3 s hosts of seeds 0 .. 19 (120 symbols of
    each kind, the best of 1024 candidates each): every z_d < 5.5 and no id."""
    for seed in range(20):
        for n in (RATE, 3 * RATE):
            x = ref.host(n, seed)
            for kind, clip in (("key-only", wave_codec.mark_pcm16(x, KEY)), ("unmarked", x), ("other key", wave_codec.mark_pcm16(x, WatermarkTag(2, IDS[seed % 12])))):
                zs = [z for _, z in _symbols(clip)]
                got = _read(clip)
                assert max(zs) < 5.5 and got.id is None and got.id_z == min(zs), (kind, seed, n, zs)
                assert got.detected == (kind == "key-only")


# ------------------------------------------------------------------------------------------------ through the layers
def test_request_options_take_tags():
    check = serve.check_request_options
    assert check(dict(watermark={"key": 7, "id": 3})) == dict(watermark=WatermarkTag(7, 3)) and check(dict(watermark=77)) == dict(watermark=77)
    assert check(dict(watermark={"id": 3}), watermark=9) == dict(watermark=WatermarkTag(9, 3))
    with pytest.raises(ValueError, match="id without a key"):
        check(dict(watermark={"id": 3}))
    with pytest.raises(ValueError, match="watermark id must be an integer from 0 to 2\\^30 - 1"):
        check(dict(watermark={"key": 7, "id": 2 ** 30}))
    assert infer.REQUEST_OPTIONS.index("watermark") == 11 and serve.EDIT_MARK == ("watermark",)      # the id rides inside the value
    tag = dict(watermark=WatermarkTag(5, 1))
    assert infer.needs_whole_wave(tag) and infer.whole_wave_message(tag) == infer.WHOLE_WAVE_WATERMARK
    assert serve.stream_refusal(tag) == serve.STREAM_WATERMARK == serve.stream_refusal(dict(watermark={"key": 5, "id": 1}))


def test_finish_requests_and_finish_pcm16_take_tags():
    fade = infer.cross_fade_duration
    rng = np.random.default_rng(9)
    reqs = [[(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens] for lens in ([20000], [15000, 14000], [9000])]
    texts, flags = ["x"] * 3, [False] * 3
    plain = infer.finish_requests(reqs, texts, fade, flags, want="pcm16")
    got = infer.finish_requests(reqs, texts, fade, flags, watermark=[WatermarkTag(5, 77), None, {"key": 6, "id": 1023}], loudness=[None, None, -20.0])
    assert got[0].dtype == np.int16 and np.array_equal(got[0], wave_codec.mark_pcm16(plain[0], WatermarkTag(5, 77)))
    assert got[1].dtype == np.float32 and np.array_equal(got[1], infer.finish_requests(reqs, texts, fade, flags)[1])
    assert np.array_equal(got[2], infer.normalise_loudness_pcm16(wave_codec.mark_pcm16(plain[2], WatermarkTag(6, 1023)), -20.0))
    for one in (WatermarkTag(5, 77), {"key": 5, "id": 77}):                                          # one tag for all: a tag is one value
        assert all(np.array_equal(g, wave_codec.mark_pcm16(x, WatermarkTag(5, 77))) for g, x in zip(infer.finish_requests(reqs, texts, fade, flags, watermark=one), plain))
    with pytest.raises(ValueError, match="watermark id must be"):
        infer.finish_requests(reqs, texts, fade, flags, watermark={"key": 5, "id": -1})
    with pytest.raises(ValueError, match="id without a key"):
        infer.finish_requests(reqs, texts, fade, flags, watermark=[{"id": 5}, None, None])
    with pytest.raises(ValueError) as e:
        infer.finish_requests([reqs[0]], [["head"]], fade, watermark=WatermarkTag(5, 77))            # a list of chunk texts
    assert str(e.value) == infer.WHOLE_WAVE_WATERMARK
    x = ref.host(2 * RATE, 4)
    spec = infer.WaveSpec.of(dict(tempo=1.25, loudness=-20.0))
    want = infer.normalise_loudness_pcm16(wave_codec.mark_pcm16(wave_codec.shift_pcm16(x, spec.tempo, spec.pitch), WatermarkTag(9, 4)), -20.0)
    assert np.array_equal(infer.finish_pcm16(x, dataclasses.replace(spec, watermark=WatermarkTag(9, 4))), want)


def test_planner_carries_the_tag(tmp_path):
    voice = infer.PreparedVoice(_voice(tmp_path))
    plan = lambda text, opts: infer.plan_request((voice, "reference words", text, opts), DEFAULTS, target_rms=0.1, fix_duration=None, device=None,   # noqa: E731
                                                 tokenizer=infer.text_to_tokens)
    assert plan("some text.", dict(watermark={"key": 5, "id": 8})).spec.watermark == WatermarkTag(5, 8) == plan("some text.", dict(watermark=WatermarkTag(5, 8))).spec.watermark
    assert plan("some text.", dict(watermark=5)).spec.watermark == 5
    assert dataclasses.replace(plan("some text.", dict(watermark={"key": 5, "id": 8})).spec, watermark=None) == infer.WaveSpec()   # a tag leaves every other field at its default
    with pytest.raises(ValueError) as e:
        plan(["one chunk.", "another chunk."], dict(watermark={"key": 5, "id": 8}))
    assert str(e.value) == infer.WHOLE_WAVE_WATERMARK
    with pytest.raises(ValueError, match="id without a key"):
        plan("some text.", dict(watermark={"id": 8}))
    from test_serve import FakeModel, FakeVocoder
    with pytest.raises(ValueError) as e:
        infer.infer_requests([(voice, "reference words", "some text.", dict(watermark=WatermarkTag(5, 8)))], FakeModel(), FakeVocoder(), nfe_step=4, join=False)
    assert str(e.value) == infer.WHOLE_WAVE_WATERMARK


def test_span_scheduler_carries_the_tag():
    import test_spans as spans
    voice = spans._voice()
    text = "This is sentence one, quite long. And here is the second sentence, also long. A third one follows. " * 3
    _, sched = spans._scheduler(span_steps=2, nfe_step=4)
    plain, marked = sched.admit(spans._request(voice, text, seed=1)), sched.admit(spans._request(voice, text, seed=1, watermark={"key": 17, "id": 4}))
    assert marked.spec.watermark == WatermarkTag(17, 4)
    while sched.busy:
        sched.step()
    assert np.array_equal(marked.result, wave_codec.mark_pcm16(infer.quantise_pcm16(plain.result), WatermarkTag(17, 4)))


def test_manager_and_speech_routes(client, tmp_path):
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    pcm = infer.quantise_pcm16(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text))
    tag = WatermarkTag(41, 123456)
    want = wave_codec.mark_pcm16(pcm, tag)
    got = mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, watermark={"key": 41, "id": 123456})
    assert got.dtype == np.int16 and np.array_equal(got, want) and not np.array_equal(want, wave_codec.mark_pcm16(pcm, 41))
    assert np.array_equal(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, watermark=tag), want)
    with pytest.raises(ValueError, match="id without a key"):                                        # no key anywhere
        mgr.synthesize(TEXT, voice.audio_path, voice.ref_text, watermark={"id": 5})
    raw = open(_voice(tmp_path), "rb").read()
    clip_pcm = infer.quantise_pcm16(mgr.synthesize_clip(TEXT, raw, "reference words"))
    assert np.array_equal(mgr.synthesize_clip(TEXT, raw, "reference words", watermark=tag), wave_codec.mark_pcm16(clip_pcm, tag))
    for stream in (mgr.synthesize_stream, lambda *a, **kw: mgr.synthesize_clip_stream(TEXT, raw, "reference words", **kw)):
        with pytest.raises(ValueError) as e:
            stream(TEXT, voice.audio_path, voice.ref_text, watermark={"key": 41, "id": 1})
        assert str(e.value) == serve.STREAM_WATERMARK
    body = dict(text=TEXT, watermark={"key": 41, "id": 123456})
    clone = dict(body, ref_audio=base64.b64encode(raw).decode(), ref_text="reference words")
    for route, extra in (("/v1/audio/speech", body), ("/v1/audio/speech/voice", dict(body, ref_audio_name="KAN_F (Happy)")), ("/v1/audio/speech/clone", clone)):
        r = c.post(route, json=dict(extra, response_format="pcm"))
        assert r.status_code == 200 and r.content == (want if "clone" not in route else wave_codec.mark_pcm16(clip_pcm, tag)).tobytes(), route
        r = c.post(route, json=dict(extra, stream=True))
        assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_WATERMARK, route
        for bad in (True, 1.0, "5", -1, 2 ** 30):
            r = c.post(route, json=dict(extra, watermark={"key": 41, "id": bad}))
            assert r.status_code == 400 and "watermark id must be an integer from 0 to 2^30 - 1" in r.json()["detail"], (route, bad)
        r = c.post(route, json=dict(extra, watermark={"key": 41, "id": 1, "tenant": 3}))
        assert r.status_code == 400 and "'tenant'" in r.json()["detail"], route
        r = c.post(route, json=dict(extra, watermark={"id": 1}))
        assert r.status_code == 400 and "id without a key" in r.json()["detail"], route
        for bad in (True, 1.0, "41", 0, 2 ** 48):                                                    # the pinned messages stay
            r = c.post(route, json=dict(extra, watermark=bad))
            assert r.status_code == 400 and "watermark must be an integer key" in r.json()["detail"], (route, bad)


def test_manager_default_tag(client):
    c, mgr, reg = client
    voice = reg.get("KAN_F (Happy)")
    pcm = infer.quantise_pcm16(mgr.synthesize(TEXT, voice.audio_path, voice.ref_text))
    for default in ({"key": 99, "id": 7}, WatermarkTag(99, 7)):                                      # e.g. one id per deployment
        marked = serve.TTSManager(nfe_step=4, watermark=default).load(mgr.model_obj, mgr.vocoder)
        assert marked.watermark == WatermarkTag(99, 7)
        assert np.array_equal(marked.synthesize(TEXT, voice.audio_path, voice.ref_text), wave_codec.mark_pcm16(pcm, WatermarkTag(99, 7)))
        assert np.array_equal(marked.synthesize(TEXT, voice.audio_path, voice.ref_text, watermark={"id": 8}), wave_codec.mark_pcm16(pcm, WatermarkTag(99, 8)))
        assert np.array_equal(marked.synthesize(TEXT, voice.audio_path, voice.ref_text, watermark=5), wave_codec.mark_pcm16(pcm, 5))   # the request's own key wins
        with pytest.raises(ValueError) as e:
            marked.synthesize_stream(TEXT, voice.audio_path, voice.ref_text)
        assert str(e.value) == serve.STREAM_WATERMARK
    keyed = serve.TTSManager(nfe_step=4, watermark=99).load(mgr.model_obj, mgr.vocoder)              # a plain key completes an id too
    assert np.array_equal(keyed.synthesize(TEXT, voice.audio_path, voice.ref_text, watermark={"id": 8}), wave_codec.mark_pcm16(pcm, WatermarkTag(99, 8)))
    for bad in ({"id": 7}, {"key": 99, "id": 2 ** 30}, {"key": 99, "x": 1}):
        with pytest.raises(ValueError, match="watermark"):
            serve.TTSManager(watermark=bad)


def test_script_route_and_method(script_client):
    c, mgr, path = script_client
    mgr.load(NoiseModel(), Vocoder())
    voices = dict(main=dict(ref_audio_path=path, ref_text=RA), town=dict(ref_audio=_wav(B), ref_text=RB))
    pcm = infer.quantise_pcm16(mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4))
    want = wave_codec.mark_pcm16(pcm, WatermarkTag(12, 900))
    got = mgr.synthesize_script(SCRIPT, voices, gap=0.5, seed=4, watermark={"key": 12, "id": 900})
    assert got.dtype == np.int16 and np.array_equal(got, want)
    with pytest.raises(ValueError) as e:
        mgr.synthesize_script_stream(SCRIPT, voices, watermark={"key": 12, "id": 900})
    assert str(e.value) == serve.STREAM_WATERMARK
    town = dict(ref_audio=base64.b64encode(_wav(B)).decode(), ref_text=RB)
    body = dict(text=SCRIPT, voices=dict(main=dict(ref_audio_name="KAN_F (Happy)"), town=town), seed=4, gap=0.5, watermark={"key": 12, "id": 900})
    r = c.post("/v1/audio/speech/script", json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
    r = c.post("/v1/audio/speech/script", json=dict(body, stream=True))
    assert r.status_code == 400 and r.json()["detail"] == serve.STREAM_WATERMARK
    r = c.post("/v1/audio/speech/script", json=dict(body, watermark={"key": 12, "id": "900"}))
    assert r.status_code == 400 and "watermark id must be" in r.json()["detail"]


def test_edit_route_and_method(client, tmp_path, monkeypatch):
    c, mgr, _ = client
    raw = open(_voice(tmp_path), "rb").read()
    edited = (ref.host(3 * RATE, 5).astype(np.float32) / 32768.0)
    monkeypatch.setattr(infer, "speech_edit_batch", lambda edits, *a, **kw: [(edited, RATE, None)] * len(edits))
    want = wave_codec.mark_pcm16(infer.quantise_pcm16(edited), WatermarkTag(8, 31337))                # the whole returned recording, on the host
    got = mgr.edit(raw, "new words", [[0.2, 0.5]], watermark={"key": 8, "id": 31337})
    assert got.dtype == np.int16 and np.array_equal(got, want) and _read(got, 8).id == 31337
    body = dict(audio=base64.b64encode(raw).decode(), text="new words", parts_to_edit=[[0.2, 0.5]], watermark={"key": 8, "id": 31337})
    r = c.post("/v1/audio/edit", json=dict(body, response_format="pcm"))
    assert r.status_code == 200 and r.content == want.tobytes()
    r = c.post("/v1/audio/edit", json=dict(body, watermark={"key": 8, "id": 1.5}))
    assert r.status_code == 400 and "watermark id must be" in r.json()["detail"]


def test_read_method_and_detect_route(client):
    c, mgr, _ = client
    y = wave_codec.mark_pcm16(ref.host(3 * RATE, 6), WatermarkTag(31, 424242))
    reads = mgr.read_watermark(_wav24(y), [31, 32])                                                  # no model on a GPU: the host, fp64
    assert reads == wave_codec.read_watermark(y.astype(np.float32) / np.float32(32768.0), [31, 32])
    assert [r.id for r in reads] == [424242, None] and [r.detected for r in reads] == [True, False]
    assert [tuple(r)[:4] for r in reads] == [tuple(s) for s in mgr.detect_watermark(_wav24(y), [31, 32])]
    assert [r.id for r in mgr.read_watermark(infer.encode_flac(y, RATE).tobytes(), [31])] == [424242]
    with pytest.raises(ValueError, match="read_watermark needs keys"):
        mgr.read_watermark(_wav24(y))
    for default in (31, {"key": 31, "id": 5}):                                                       # keys=None: the manager's own key
        own = serve.TTSManager(watermark=default)
        assert own.read_watermark(_wav24(y)) == reads[:1] and own.detect_watermark(_wav24(y)) == mgr.detect_watermark(_wav24(y), [31])
    body = dict(audio=base64.b64encode(_wav24(y)).decode(), keys=[31, 32])
    plain = c.post("/v1/audio/watermark/detect", json=body)
    assert plain.status_code == 200 and all(set(d) == {"key", "detected", "score", "offset"} for d in plain.json()["results"])   # as it is today
    assert c.post("/v1/audio/watermark/detect", json=dict(body, ids=False)).json() == plain.json()
    r = c.post("/v1/audio/watermark/detect", json=dict(body, ids=True))
    assert r.status_code == 200
    results = r.json()["results"]
    assert [set(d) for d in results] == [{"key", "detected", "score", "offset", "id", "id_score"}] * 2
    assert [(d["key"], d["detected"], d["offset"], d["id"]) for d in results] == [(31, True, 0, 424242), (32, False, reads[1].offset, None)]
    assert results[0]["id_score"] == pytest.approx(reads[0].id_z, abs=1e-12) and results[0]["score"] == pytest.approx(reads[0].z, abs=1e-12)
    assert [{k: d[k] for k in ("key", "detected", "score", "offset")} for d in results] == plain.json()["results"]
    for bad, words in ((dict(body, ids="yes"), "ids must be true or false"), (dict(body, ids=1), "ids must be true or false"),
                       (dict(body, ids=True, keys=[{"key": 31, "id": 1}]), "integer key")):
        r = c.post("/v1/audio/watermark/detect", json=bad)
        assert r.status_code == 400 and words in r.json()["detail"], r.json()


def test_reject_marked_sees_a_tagged_clip(tmp_path):
    from test_serve import FakeModel, FakeVocoder
    tagged = wave_codec.mark_pcm16(ref.host(3 * RATE, 7), WatermarkTag(21, 99))                       # a tagged clip still carries the key's mark
    mgr = serve.TTSManager(nfe_step=4, reject_marked=[20, 21], device_frontend=False).load(FakeModel(), FakeVocoder())
    with pytest.raises(ValueError) as e:
        mgr.synthesize_clip(TEXT, _wav24(tagged), "reference words")
    assert str(e.value) == serve.MARKED_REFERENCE
