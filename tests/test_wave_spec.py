"""`wave_codec.WaveSpec` (the five delivery options, the two prosody options, the watermark and `keep_formants` as one value), `infer.finish_pcm16` (the host definition of "finish this PCM") and
`wave_codec.StreamDelivery` (the same, piece by piece) against the separate validators and functions they are made of (CPU).

Every comparison is equality of values, messages and bytes."""
import dataclasses
import itertools

import numpy as np
import pytest

from tts_indic_server_f5_amd import audio_prep, infer, wave_codec as W

RATES, ENCODINGS = W.OUTPUT_SAMPLE_RATES, W.ALL_ENCODINGS
COMBINATIONS = list(itertools.product(RATES, ENCODINGS, (None, 0, 1), (None, -40, -16, -5), (None, False, True)))


def _options(rate, enc, level, loud, cut):
    return dict(sample_rate=rate, encoding=enc, flac_level=level, loudness=loud, remove_silence=cut, speed=1.0, seed=None)   # (other keys are ignored)


def test_of_equals_the_separate_validators_on_every_combination():
    assert W.DELIVERY_OPTIONS == ("remove_silence", "loudness", "sample_rate", "encoding", "flac_level")
    assert W.WaveSpec() == W.WaveSpec.of({}) == W.WaveSpec(False, None, 24000, "pcm16", 0)
    for rate, enc, level, loud, cut in COMBINATIONS:
        opts = _options(rate, enc, level, loud, cut)
        if level is not None and enc != "flac":
            with pytest.raises(ValueError) as e:
                W.WaveSpec.of(opts)
            assert str(e.value) == f"flac_level needs encoding 'flac' (got flac_level {level!r} with encoding {enc!r})"
            with pytest.raises(ValueError) as e2:
                W.request_flac_level(level, enc)
            assert str(e2.value) == str(e.value)
            continue
        spec = W.WaveSpec.of(opts)
        assert spec == W.WaveSpec(bool(cut), W.check_loudness(loud), *W.delivery_format(rate, enc), W.request_flac_level(level, enc))
        assert (spec.remove_silence, spec.loudness, spec.sample_rate, spec.encoding, spec.flac_level) == \
            (cut is True, None if loud is None else float(loud), rate, enc, level or 0)
        assert type(spec.remove_silence) is bool and type(spec.sample_rate) is int and type(spec.flac_level) is int
        assert spec.format == (rate, enc) and spec.plain_format == ((rate, enc) == (24000, "pcm16")) and spec.flac == (enc == "flac")
        assert spec.gain_constant == (None if loud is None else W.loudness_gain_constant(loud))
    with pytest.raises(AttributeError):
        spec.encoding = "alaw"                                                        # frozen


def test_missing_keys_and_none_are_the_defaults():
    assert W.WaveSpec.of(dict(sample_rate=None, encoding=None, flac_level=None, loudness=None, remove_silence=None)) == W.WaveSpec()
    assert W.WaveSpec.of(dict(encoding="flac")) == W.WaveSpec(encoding="flac") and W.WaveSpec.of(dict(sample_rate=np.int64(8000))).sample_rate == 8000
    assert W.WaveSpec.of(dict(loudness=-16)).loudness == -16.0 and W.WaveSpec.of(dict(encoding="flac", flac_level=np.int32(1))).flac_level == 1


REFUSALS = [
    (dict(flac_level=1, encoding="alaw"), "flac_level needs encoding 'flac' (got flac_level 1 with encoding 'alaw')"),
    (dict(flac_level=0), "flac_level needs encoding 'flac' (got flac_level 0 with encoding None)"),
    (dict(flac_level=True, encoding="flac"), "flac_level must be one of [0, 1] (got True)"),
    (dict(flac_level="1", encoding="flac"), "flac_level must be one of [0, 1] (got '1')"),
    (dict(flac_level=2, encoding="flac"), "flac_level must be one of [0, 1] (got 2)"),
    (dict(sample_rate=True), "sample_rate must be one of [8000, 16000, 22050, 24000, 32000, 44100, 48000] (got True)"),
    (dict(sample_rate=11025), "sample_rate must be one of [8000, 16000, 22050, 24000, 32000, 44100, 48000] (got 11025)"),
    (dict(sample_rate="8000"), "sample_rate must be one of [8000, 16000, 22050, 24000, 32000, 44100, 48000] (got '8000')"),
    (dict(encoding="mp3"), "encoding must be one of ['pcm16', 'mulaw', 'alaw', 'flac'] (got 'mp3')"),
    (dict(loudness=-41), "loudness must be between -40 and -5 LUFS (got -41.0)."),
    (dict(loudness=-4.5), "loudness must be between -40 and -5 LUFS (got -4.5)."),
    (dict(loudness=float("nan")), "loudness must be between -40 and -5 LUFS (got nan)."),
    (dict(loudness=True), "loudness must be a number of LUFS (got True)"),
    (dict(loudness="-16"), "loudness must be a number of LUFS (got '-16')"),
    # two at once: loudness, then the level, then the format -- the order of `plan_request`
    (dict(loudness=0, flac_level=1, encoding="mp3"), "loudness must be between -40 and -5 LUFS (got 0.0)."),
    (dict(flac_level=1, encoding="mp3"), "flac_level needs encoding 'flac' (got flac_level 1 with encoding 'mp3')"),
    (dict(flac_level=3, sample_rate=1), "flac_level must be one of [0, 1] (got 3)"),
    # the other four of the nine (the strings of tests/test_prosody_host.py, test_watermark_host.py, test_watermark_id_host.py, test_formant_host.py)
    (dict(tempo=True), "tempo must be a number from 0.5 to 2 in steps of 0.01 (got True)"),
    (dict(tempo=2.01), "tempo must be a number from 0.5 to 2 in steps of 0.01 (got 2.01)"),
    (dict(tempo="1.0"), "tempo must be a number from 0.5 to 2 in steps of 0.01 (got '1.0')"),
    (dict(pitch=7), "pitch must be a whole number of semitones from -6 to 6 (got 7)"),
    (dict(pitch=1.0), "pitch must be a whole number of semitones from -6 to 6 (got 1.0)"),
    (dict(pitch=True), "pitch must be a whole number of semitones from -6 to 6 (got True)"),
    (dict(tempo=0.5, pitch=3), "tempo 0.5 with pitch 3 stretches the wave by 88/37: outside 1/2 to 2"),
    (dict(watermark=True), "watermark must be an integer key from 1 to 2^48 - 1 (got True)"),
    (dict(watermark=1.5), "watermark must be an integer key from 1 to 2^48 - 1 (got 1.5)"),
    (dict(watermark="7"), "watermark must be an integer key from 1 to 2^48 - 1 (got '7')"),
    (dict(watermark=0), "watermark must be an integer key from 1 to 2^48 - 1 (got 0)"),
    (dict(watermark=2 ** 48), f"watermark must be an integer key from 1 to 2^48 - 1 (got {2 ** 48})"),
    (dict(watermark={"key": 0, "id": 1}), "watermark must be an integer key from 1 to 2^48 - 1 (got 0)"),
    (dict(watermark={"key": 7, "id": 2 ** 30}), f"watermark id must be an integer from 0 to 2^30 - 1 (got {2 ** 30})"),
    (dict(watermark={"key": 7, "id": True}), "watermark id must be an integer from 0 to 2^30 - 1 (got True)"),
    (dict(watermark={"key": 7, "id": 1, "tenant": 3}), "watermark has an unknown entry 'tenant': a key with a trace id is {\"key\": K, \"id\": I}"),
    (dict(watermark={"id": 3}), "watermark names an id without a key, and the service has no key of its own (got {'id': 3})"),   # only `serve` knows a default key
    (dict(pitch=2, keep_formants=1), "keep_formants must be true or false (got 1)"),
    (dict(pitch=2, keep_formants="true"), "keep_formants must be true or false (got 'true')"),
    (dict(keep_formants=True), "keep_formants needs a non-zero pitch"),
    (dict(keep_formants=True, pitch=0, tempo=1.25), "keep_formants needs a non-zero pitch"),
    # two at once, within one request: the five, the tempo, the pitch, their stretch, then the key, then the flag
    (dict(loudness=True, watermark=True), "loudness must be a number of LUFS (got True)"),
    (dict(pitch=9, watermark=True, keep_formants=1), "pitch must be a whole number of semitones from -6 to 6 (got 9)"),
    (dict(tempo=0.5, pitch=3, watermark=0, keep_formants=True), "tempo 0.5 with pitch 3 stretches the wave by 88/37: outside 1/2 to 2"),
    (dict(watermark=0, keep_formants=True), "watermark must be an integer key from 1 to 2^48 - 1 (got 0)"),
]


@pytest.mark.parametrize("opts,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_character_for_character(opts, message):
    for call in (W.WaveSpec.of, infer.needs_whole_wave, infer.whole_wave_message):
        with pytest.raises(ValueError) as e:
            call(opts)
        assert str(e.value) == message
    with pytest.raises(ValueError) as e:
        infer.plan_request((None, "", "x", opts), {}, target_rms=0.1, fix_duration=None, device=None, tokenizer=None)
    assert str(e.value) == message


def test_which_message_wins_where_two_things_are_bad_at_once():
    """The order of the checks around the spec, as it was before there was one."""
    from tts_indic_server_f5_amd import serve
    wave = [[np.zeros(100, dtype=np.float32)]]
    with pytest.raises(ValueError, match='^want must be "float" or "pcm16"'):
        infer.finish_requests(wave, [""], want="int8", sample_rate=1, loudness=0)
    with pytest.raises(ValueError, match="^the device back-end produces int16 PCM"):
        infer.finish_requests(wave, [""], device_backend=True, encoding="mp3")
    with pytest.raises(ValueError, match="^finish_requests: one sample_rate or one per request"):
        infer.finish_requests(wave, [""], sample_rate=[8000, 8000], loudness=0)
    # the edit route hands its fields over in this order: the sampler's, then sample_rate, encoding, loudness
    assert serve.EDIT_DELIVERY == ("sample_rate", "encoding", "loudness", "flac_level")
    allowed = tuple(dict.fromkeys(serve.EDIT_OPTIONS + serve.EDIT_DELIVERY))
    assert allowed == serve.EDIT_OPTIONS + ("sample_rate", "encoding", "loudness")
    bad = dict.fromkeys(allowed) | dict(flac_level=True, sample_rate=1, encoding="mp3", loudness=0)
    for name in ("flac_level", "sample_rate", "encoding", "loudness"):             # each option's own message, in that order
        with pytest.raises(ValueError, match=f"^{name} must be"):
            serve.check_request_options(bad, allowed=allowed)
        bad[name] = None
    with pytest.raises(ValueError, match="^flac_level needs encoding 'flac'"):       # the options together: after each one alone
        serve.check_request_options(dict(flac_level=1, encoding="alaw"), allowed=allowed)


def test_whole_wave_rule_on_every_combination():
    """The rule, written out: silence removal and a loudness target always need the whole wave; a format other than 24 kHz pcm16 does unless
    the request is streamed (its owner applies the format to the pieces).  The message names loudness only when there is a target and no
    silence removal."""
    assert infer.WHOLE_WAVE is W.WHOLE_WAVE and infer.WHOLE_WAVE_LOUDNESS is W.WHOLE_WAVE_LOUDNESS
    assert infer.WHOLE_WAVE.startswith("remove_silence, sample_rate and encoding need the request's whole wave: they are not available for a list")
    assert infer.WHOLE_WAVE_LOUDNESS.startswith("loudness is measured on the request's whole wave: it is not available for a list of chunk texts")
    for rate, enc, level, loud, cut in COMBINATIONS:
        if level is not None and enc != "flac":
            continue
        opts = _options(rate, enc, level, loud, cut)
        for streamed in (False, True):
            want = cut is True or loud is not None or (not streamed and (rate, enc) != (24000, "pcm16"))
            assert infer.needs_whole_wave(opts, streamed=streamed) is want, (opts, streamed)
            assert W.WaveSpec.of(opts).needs_whole_wave(streamed) is want
        assert infer.needs_whole_wave(opts) is W.WaveSpec.of(opts).needs_whole_wave()
        message = infer.WHOLE_WAVE_LOUDNESS if loud is not None and cut is not True else infer.WHOLE_WAVE
        assert infer.whole_wave_message(opts) == W.WaveSpec.of(opts).whole_wave_message() == message


def test_wave_options_are_the_fields_and_the_four_tuples():
    names = tuple(f.name for f in dataclasses.fields(W.WaveSpec))
    assert W.WAVE_OPTIONS == infer.WAVE_OPTIONS == names == W.DELIVERY_OPTIONS + W.PROSODY_OPTIONS + W.WATERMARK_OPTIONS + W.FORMANT_OPTIONS
    assert len(names) == 9 and set(names) == set(infer.REQUEST_OPTIONS[6:])
    spec = W.WaveSpec(True, -16.0, 8000, "mulaw", 0, 1.25, 2)                          # the seven-argument positional form keeps its meaning
    assert (spec.tempo, spec.pitch, spec.watermark, spec.keep_formants) == (1.25, 2, None, False)
    assert W.WaveSpec.of(dict(watermark={"key": 5, "id": 8})) == W.WaveSpec(watermark=W.WatermarkTag(5, 8)) == W.WaveSpec.of(dict(watermark=W.WatermarkTag(5, 8)))
    assert W.WaveSpec.of(dict(watermark={"key": 5})) == W.WaveSpec(watermark=5) == W.WaveSpec.of(dict(watermark=np.int64(5)))
    assert W.WaveSpec.of(dict(watermark=None, keep_formants=None)) == W.WaveSpec()


MARKS = (None, 5, W.WatermarkTag(5, 8), {"key": 5, "id": 8})
# every other reason alone: (options, whether it counts for a streamed request, its message without a mark)
REASONS = [
    (dict(), None, None),
    (dict(remove_silence=True), True, W.WHOLE_WAVE),
    (dict(loudness=-20.0), True, W.WHOLE_WAVE_LOUDNESS),
    (dict(tempo=1.25), True, W.WHOLE_WAVE_PROSODY),
    (dict(pitch=-2), True, W.WHOLE_WAVE_PROSODY),
    (dict(pitch=2, keep_formants=True), True, W.WHOLE_WAVE_PROSODY),
    (dict(sample_rate=8000), False, W.WHOLE_WAVE),
    (dict(encoding="flac", flac_level=1), False, W.WHOLE_WAVE),
    (dict(loudness=-20.0, remove_silence=True), True, W.WHOLE_WAVE),
    (dict(tempo=1.25, loudness=-20.0), True, W.WHOLE_WAVE_LOUDNESS),
]


def test_a_mark_in_the_whole_wave_rule():
    """A mark always needs the whole wave, streamed or not, and it has the message exactly when it is the only reason; `infer`'s two
    functions of a dict of options are the spec's."""
    for reason, streamed_too, message in REASONS:
        for mark in MARKS:
            opts = dict(reason, watermark=mark, speed=1.0)
            spec = W.WaveSpec.of(opts)
            for streamed in (False, True):
                want = mark is not None or (message is not None and (streamed_too or not streamed))
                assert infer.needs_whole_wave(opts, streamed) is spec.needs_whole_wave(streamed) is want, (opts, streamed)
            if mark is None and message is None:
                continue   # (nothing to refuse)
            only = mark is not None and message is None
            assert infer.whole_wave_message(opts) == spec.whole_wave_message() == (W.WHOLE_WAVE_WATERMARK if only else message), opts
            assert (spec.whole_wave_message() == W.WHOLE_WAVE_WATERMARK) == only


def test_the_stretch_is_the_tempos_alone_with_keep_formants():
    assert W.WaveSpec.of(dict(tempo=1.25, pitch=2, keep_formants=True)).stretch == W.formant_stretch(125) == (4, 5)
    assert W.WaveSpec.of(dict(tempo=1.25, pitch=2)).stretch == W.prosody_stretch(125, 2) == (184, 205)
    assert W.WaveSpec.of(dict(pitch=2, keep_formants=True)).stretch == (1, 1)


def test_key_and_flag_count_in_equality_and_hash():
    base = W.WaveSpec.of(dict(tempo=1.25, pitch=2, loudness=-20.0))
    others = [dataclasses.replace(base, watermark=5), dataclasses.replace(base, watermark=6), dataclasses.replace(base, watermark=W.WatermarkTag(5, 0)),
              dataclasses.replace(base, watermark=W.WatermarkTag(5, 1)), dataclasses.replace(base, keep_formants=True),
              dataclasses.replace(base, watermark=5, keep_formants=True)]
    specs = [base] + others
    assert len(set(specs)) == len(specs) == len({hash(s) for s in specs})
    assert all(a != b for a, b in itertools.combinations(specs, 2))
    table = {W.WaveSpec.of(dict(watermark={"key": 5, "id": 1})): "tagged"}                # a spec with a tag is a dict key
    assert table[W.WaveSpec(watermark=W.WatermarkTag(5, 1))] == "tagged" and W.WaveSpec(watermark=5) not in table
    with pytest.raises(AttributeError):
        base.watermark = 5                                                            # frozen


def _paused_pcm():
    """The paused request of tests/test_gpu_finish_mixed.py, joined and quantised: 44400 samples with a pause of 27000."""
    rng = np.random.default_rng(0)
    a, b = (rng.uniform(-0.2, 0.2, n).astype(np.float32) for n in (36000, 12000))
    a[6000:33000] = 0.0
    return infer.quantise_pcm16(infer.request_wave("", [a, b], infer.cross_fade_duration))


def test_finish_pcm16_is_the_three_step_composition():
    pcm = _paused_pcm()
    assert pcm.dtype == np.int16 and len(pcm) == 44400
    cut = audio_prep.remove_silence_pcm(pcm, 24000)
    assert len(cut) < len(pcm)
    assert infer.finish_pcm16(pcm, W.WaveSpec()) is pcm
    for opts in (dict(remove_silence=True), dict(loudness=-20), dict(remove_silence=True, loudness=-16, sample_rate=8000, encoding="mulaw"),
                 dict(sample_rate=16000), dict(remove_silence=True, encoding="flac", flac_level=1, sample_rate=16000), dict(loudness=-30, encoding="flac")):
        x = cut if opts.get("remove_silence") else pcm
        x = W.normalise_loudness_pcm16(x, opts.get("loudness"))
        want = W.deliver_pcm16(x, opts.get("sample_rate"), opts.get("encoding"), opts.get("flac_level"))
        got = infer.finish_pcm16(pcm, W.WaveSpec.of(opts))
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), opts
        host, = infer.finish_requests([[pcm.astype(np.float32) / 32768.0]], [""], want="pcm16", remove_silence=[bool(opts.get("remove_silence"))],
                                      sample_rate=opts.get("sample_rate"), encoding=opts.get("encoding"), loudness=opts.get("loudness"),
                                      flac_level=opts.get("flac_level"))
        assert host.dtype == want.dtype and host.tobytes() == want.tobytes(), opts


# ------------------------------------------------------------------------------------------------ StreamDelivery
@pytest.fixture(scope="module")
def stream():
    """3 s of full-scale noise as float32, its int16 PCM, and the pieces: cut at 20 points -- two empty pieces, one of 5 samples (shorter
    than any resampler tile) and one of 30000 (more than two FLAC blocks at every rate)."""
    rng = np.random.default_rng(1)
    wave = rng.uniform(-1.0, 1.0, 72000).astype(np.float32)
    cuts = sorted(rng.choice(np.arange(30006, 72000), size=16, replace=False).tolist())
    cuts = [5, 5, 30005] + cuts[:8] + [cuts[7]] + cuts[8:]
    assert len(cuts) == 20 and cuts == sorted(cuts)
    pieces = [wave[a:b] for a, b in zip([0] + cuts, cuts + [len(wave)])]
    assert sum(len(p) == 0 for p in pieces) == 2 and min(len(p) for p in pieces if len(p)) == 5 and max(len(p) for p in pieces) == 30000
    assert 30000 * 8000 // 24000 > 2 * W.FLAC_BLOCK
    return W.quantise_pcm16(wave), pieces


def _streamed(spec, pieces):
    delivery = W.StreamDelivery(spec)
    out = [o for piece in pieces for o in delivery.feed(piece)] + delivery.finish()
    assert all(len(o) for o in out)                                                  # no empty output piece
    return out


@pytest.mark.parametrize("enc", W.OUTPUT_ENCODINGS)
def test_stream_delivery_equals_deliver_pcm16_byte_for_byte(stream, enc):
    pcm, pieces = stream
    for rate in RATES:
        if (rate, enc) == (24000, "pcm16"):
            continue
        spec = W.WaveSpec(sample_rate=rate, encoding=enc)
        out = _streamed(spec, pieces)
        want = W.deliver_pcm16(pcm, rate, enc)
        assert all(o.dtype == want.dtype for o in out)
        assert np.concatenate(out).tobytes() == want.tobytes(), (rate, enc)
        assert _streamed(spec, []) == []                                             # a stream without a piece: nothing


@pytest.mark.parametrize("level", W.FLAC_LEVELS)
def test_stream_delivery_flac_header_first_then_the_whole_ones_frames(stream, level):
    pcm, pieces = stream
    for rate in RATES:
        spec = W.WaveSpec(sample_rate=rate, encoding="flac", flac_level=level)
        header = W.StreamFlacEncoder(rate, level).header()
        assert len(header) == W.FLAC_HEADER_BYTES == 42
        delivery = W.StreamDelivery(spec)
        first = delivery.feed(pieces[0])
        assert first[0].tobytes() == header                                         # in front of what the first piece releases
        out = first + [o for piece in pieces[1:] for o in delivery.feed(piece)] + delivery.finish()
        assert all(o.dtype == np.uint8 and len(o) for o in out)
        got, want = np.concatenate(out).tobytes(), W.deliver_pcm16(pcm, rate, "flac", level).tobytes()
        assert got[:42] == header and got[42:] == want[42:], (rate, level)
        bare = _streamed(spec, [])
        assert len(bare) == 1 and bare[0].tobytes() == header                       # a stream without a piece: the bare header
