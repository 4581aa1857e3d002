"""GPU: every device entry point on a caller's non-default stream (tests/stream_harness.py has the method).

Part 1: each entry gives on a fresh side stream, behind a producer that delivers its data inputs late, the bits it gives on the default
stream -- with a fresh handle whose first call ever is the side-stream call, and once more on the same handle.  One negative control shows
that the harness sees a wrong stream on this runtime: a unit op issued on the NULL stream while the producer sits on the side stream reads
the poison.
Part 3: two handle-less calls of one kind issued back to back on two streams, the first still queued behind its late producer when the
second is issued.  The calls of a kind share one per-device workspace (csrc/ragged_util.h); its turn (WorkspaceTurn) makes the second
stream wait for the first call's kernels, so each call's result is what it is alone.

Every comparison is equality of bits; there is no tolerance anywhere.  No test here captures a graph, starts a thread or a process."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref  # noqa: E402
import flac_cases  # noqa: E402
import stream_harness as H  # noqa: E402
import watermark_ref  # noqa: E402
from test_gpu_request_knobs import _backbone  # noqa: E402
from tts_indic_server_f5_amd import _lib, infer, ops, synth, torch_ops, wave_codec  # noqa: E402
from tts_indic_server_f5_amd.mel import mel_spectrogram, mel_spectrogram_bigvgan, mel_spectrogram_ragged  # noqa: E402

DEV = "cuda:0"
RATE = 24000
VOCAB = {chr(65 + i): i for i in range(40)}   # the tiny backbones' 40 token ids as characters (sample_units takes token lists)
K1, K2 = 1, 0xDEADBEEF
NONE = lambda: None   # noqa: E731  (the context of an entry without a handle)


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _p(t):
    return None if t is None else C.c_void_p(t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr())


class _ctypes_binding:
    """Forces the ctypes binding of every wrapper for the block, as test_ctypes_and_torch_op_paths_agree does"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            assert torch_ops.load()
            torch_ops._loaded = False

    def __exit__(self, *exc):
        if self.on:
            torch_ops._loaded = True


def _case(name, inputs, fresh, run, binding="default"):
    with _ctypes_binding(binding == "ctypes"):
        return H.same_bits_on_a_side_stream(f"{name} ({binding} binding)", inputs, fresh, run)


# ---------------------------------------------------------------------------------------------------------------- the negative control
def test_control_a_call_on_the_null_stream_reads_the_poison():
    """f5hip_op_layernorm (M = 8, D = 256) through ctypes with stream = NULL while its input's producer sits on the side stream behind the
    delay: the output holds NaN, so a launch on the wrong stream is visible to this harness on this runtime (torch's pool streams do not
    block against the NULL stream).  NaN is read as data and nothing else."""
    g = torch.Generator().manual_seed(1)
    real = torch.randn(8, 256, generator=g).to(DEV)
    scale, shift = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
    out = torch.zeros(8, 256, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.full_like(real, float("nan"))
        s.synchronize()
        e0, e1 = H.queue_delay(s, 100.0)
        x.copy_(real)
        produced = torch.cuda.Event()
        produced.record(s)
        assert not produced.query()
        _lib.check(_lib.lib().f5hip_op_layernorm(8, 256, _p(x), _p(scale), _p(shift), 1.0, 1e-6, 0, _p(out), C.c_void_p(0)), "f5hip_op_layernorm")
        pending = not produced.query()
    s.synchronize()
    torch.cuda.synchronize()
    print(f"[streams] control: delay {e0.elapsed_time(e1):.1f} ms, producer still pending after the NULL-stream call returned: {pending}; "
          f"{int(torch.isnan(out).sum())} of {out.numel()} outputs NaN (side stream: torch.cuda.Stream(), no stream of our own needed)")
    assert torch.isnan(out).any(), "the NULL-stream call did not read the poison: the harness cannot see a wrong stream on this runtime"


# ---------------------------------------------------------------------------------------------------------------- samplers
KINDS = ["dit", "unett", "mmdit"]
UNITS = [(24, 12, 41), (12, 10, 129)]   # (prompt frames, tokens, frames): 129 pads to 256 rows
_TOK = torch.Generator().manual_seed(30)
TEXTS = [torch.randint(0, 40, (1, nt), generator=_TOK) for _, nt, _ in UNITS]
DURS = [d for _, _, d in UNITS]


def _model(kind):
    from tts_indic_server_f5_amd.model import F5HipModel
    arch, sd, _, _ = _backbone(kind)
    return F5HipModel(arch, sd, vocab_char_map=VOCAB, gemm_planes=2)


def _sampler_inputs():
    g = torch.Generator().manual_seed(31)
    t = {}
    for i, (p, _, d) in enumerate(UNITS):
        t[f"cond{i}"] = torch.randn(1, p, 100, generator=g).to(DEV)
        t[f"y0{i}"] = torch.randn(d, 100, generator=g).to(DEV)
    return t


def _sample(model, t, **kw):
    pad = torch.nn.utils.rnn.pad_sequence
    conds = pad([t["cond0"][0], t["cond1"][0]], batch_first=True)
    texts = pad([x[0] for x in TEXTS], batch_first=True, padding_value=-1)
    out, _ = model.sample(conds, texts, torch.tensor(DURS), lens=torch.tensor([p for p, _, _ in UNITS]), y0=[t["y00"], t["y01"]],
                          sway_sampling_coef=-1.0, **kw)
    return [out[i, :d] for i, d in enumerate(DURS)]


def _sample_units(model, t):
    toks = [[chr(65 + int(i)) for i in x[0]] for x in TEXTS]
    return model.sample_units([t["cond0"], t["cond1"]], list(zip(toks, DURS)), steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0,
                              y0=[t["y00"], t["y01"]])


def _spans(model, t):
    planned = [model.plan_unit(t[f"cond{i}"], TEXTS[i][0], DURS[i], steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=t[f"y0{i}"]) for i in range(2)]
    assert model.advance(planned, 2) == []                 # the state stays on the device between the two calls on the stream
    assert model.advance(planned, 2) == planned
    return [p.mel for p in planned]


SAMPLER_ENTRIES = {
    "sample": lambda m, t: _sample(m, t, steps=3, cfg_strength=2.0),                                   # f5hip_cfm_sample_masked
    "grids_methods": lambda m, t: _sample(m, t, steps=[2, 3], cfg_strength=2.0, ode_method=["rk4", "euler"]),   # per-row time tables
    "sample_units": _sample_units,
    "spans": _spans,                                                                                   # f5hip_cfm_sample_span, twice
}
WHOLE_GRID = ("sample", "grids_methods", "sample_units")     # the entries that keep their time tables from call to call


def _sampler_case(kind, entry, binding="default"):
    """default stream twice on one handle; then a fresh handle whose first call ever is the side-stream call, and the same handle again:
    `time_table_builds` counts one build for the first whole-grid call and none for the second, as tests/test_gpu_time_table_cache.py
    finds on the default stream"""
    name, run = f"{kind} {entry} ({binding} binding)", SAMPLER_ENTRIES[entry]
    with _ctypes_binding(binding == "ctypes"):
        want, real, host_ms = H.default_stream_run(name, _sampler_inputs, lambda: _model(kind), run)
        model = _model(kind)
        torch.cuda.synchronize()
        _reset()
        got, _ = H.side_stream_run(name + " [first call of a fresh handle]", real, model, run, host_ms)
        first = _counter("time_table_builds")
        H.same(got, want, f"{name}: fresh handle on a side stream vs the default stream")
        got, _ = H.side_stream_run(name + " [second call on the handle]", real, model, run, host_ms)
        second = _counter("time_table_builds")
        H.same(got, want, f"{name}: second call on a side stream vs the default stream")
    print(f"[streams] {name}: time_table_builds {first} after the first side-stream call, {second} after the second")
    if entry in WHOLE_GRID:
        assert (first, second) == (1, 1), "the time tables were not built once and reused on the side stream"
    else:
        assert second > first > 0                # (the span entry always builds: tests/test_gpu_time_table_cache.py)


@pytest.mark.parametrize("entry", list(SAMPLER_ENTRIES))
@pytest.mark.parametrize("kind", KINDS)
def test_sampler_on_a_side_stream(kind, entry):
    _sampler_case(kind, entry)


def test_sampler_on_a_side_stream_through_ctypes():
    _sampler_case("dit", "grids_methods", "ctypes")


@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_tap_on_a_side_stream(kind):
    """transformer_forward stopped behind block 1, the text tap of that layout, the whole forward (MMDiT's tap: the token rows of the text
    slab, as tests/test_gpu_isolation.py reads it)"""
    g = torch.Generator().manual_seed(32)
    text = torch.randint(0, 40, (2, 12), generator=g)

    def inputs():
        return {"x": torch.randn(2, 41, 100, generator=g).to(DEV), "cond": torch.randn(2, 41, 100, generator=g).to(DEV)}

    def run(model, t):
        h = model.transformer_forward(t["x"], t["cond"], text, 0.37, False, False, n_blocks=1)
        if kind == "mmdit":
            rows = model.read_tap("text_rows", 256, model.arch.dim)
            tap = torch.cat([rows[0:12], rows[128:140]])
        else:
            tap = model.read_tap("text_embed", 2 * 41, model.arch.text_dim)
        return [h, tap, model.transformer_forward(t["x"], t["cond"], text, 0.37, False, False)]

    _case(f"{kind} transformer_forward + read_tap", inputs, lambda: _model(kind), run)


# ---------------------------------------------------------------------------------------------------------------- vocoders
BV_C0 = 256


def _mels(frames, seed):
    g = torch.Generator().manual_seed(seed)
    return {f"mel{i}": (torch.randn(100, t, generator=g) * 1.5 - 1.0).to(DEV) for i, t in enumerate(frames)}


@pytest.fixture(scope="module")
def voc_sd():
    return {"vocos": synth.vocos_state_dict(), "bigvgan": synth.bigvgan_state_dict(upsample_initial_channel=BV_C0)}


def _vocos(voc_sd):
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipVocos(voc_sd["vocos"], gemm_planes=2)


def _bigvgan(voc_sd):
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    return F5HipBigVGAN(voc_sd["bigvgan"], upsample_initial_channel=BV_C0, gemm_planes=2)


def _taps_run(voc, t):
    frames = [13, 2, 40]
    mel = torch.zeros(3, 100, 40, device=DEV)
    for i, f in enumerate(frames):
        mel[i, :, :f] = t[f"mel{i}"]
    out = voc.decode_taps(mel, frames)
    return [out[k] for k in ("x", "y", "fw", "wave")]


VOCODER_CASES = {
    "vocos decode": ("vocos", [13, 13], lambda v, t: [v.decode(torch.stack([t["mel0"], t["mel1"]]))]),
    "vocos decode_ragged": ("vocos", [13, 2, 40], lambda v, t: v.decode_ragged([t["mel0"], t["mel1"], t["mel2"]])),
    "vocos decode_taps": ("vocos", [13, 2, 40], _taps_run),
    "bigvgan forward": ("bigvgan", [13, 13], lambda v, t: [v(torch.stack([t["mel0"], t["mel1"]]))]),
    "bigvgan decode_ragged": ("bigvgan", [13, 1, 40], lambda v, t: v.decode_ragged([t["mel0"], t["mel1"], t["mel2"]])),
}


@pytest.mark.parametrize("name", list(VOCODER_CASES))
def test_vocoder_on_a_side_stream(voc_sd, name):
    which, frames, run = VOCODER_CASES[name]
    _case(name, lambda: _mels(frames, 40), lambda: (_vocos if which == "vocos" else _bigvgan)(voc_sd), run)


def test_vocoder_on_a_side_stream_through_ctypes(voc_sd):
    which, frames, run = VOCODER_CASES["vocos decode_ragged"]
    _case("vocos decode_ragged", lambda: _mels(frames, 40), lambda: _vocos(voc_sd), run, "ctypes")


# ---------------------------------------------------------------------------------------------------------------- the front of the model
def _noise(n, seed, amp=0.2):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("fe", [mel_spectrogram, mel_spectrogram_bigvgan], ids=["vocos", "bigvgan"])
def test_mel_front_end_on_a_side_stream(fe):
    _case(fe.__name__, lambda: {"wave": _dev(np.stack([_noise(6000, 50), _noise(6000, 51)]))}, NONE, lambda _, t: [fe(t["wave"])])


CLIPS = (1024, 4411, 24077)


def _mel_ragged_case(variant, binding="default", clips=CLIPS):
    _case(f"mel_spectrogram_ragged {variant}", lambda: {f"w{i}": _dev(_noise(n, 52 + i)) for i, n in enumerate(clips)}, NONE,
          lambda _, t: [mel_spectrogram_ragged([t[f"w{i}"] for i in range(len(clips))], variant)[0]], binding)


@pytest.mark.parametrize("variant", ["vocos", "bigvgan"])
def test_mel_ragged_on_a_side_stream(variant):
    _mel_ragged_case(variant)


def test_mel_ragged_on_a_side_stream_through_ctypes():
    _mel_ragged_case("vocos", "ctypes")


@pytest.mark.parametrize("rate", [44100, 11025], ids=["44100_table_in_lds", "11025_table_through_l2"])
def test_ref_frontend_on_a_side_stream(rate):
    n_in, ch = [3001, 1500, 7000], [1, 2, 1]
    taps = infer.resample_taps(rate, RATE)[3].to(DEV)

    def run(_, t):
        out, rms, n_out = ops.ref_frontend(t["wave"], n_in, ch, rate, RATE, taps, 0.1)
        assert out.numel() == sum(n_out)
        return [out, rms]

    _case(f"ref_frontend {rate} Hz", lambda: {"wave": _dev(_noise(sum(n * c for n, c in zip(n_in, ch)), 60, 0.05))}, NONE, run)


def test_ref_prestep_on_a_side_stream():
    """`ops.ref_prestep` takes the frames as a device tensor too: the late producer delivers them"""
    import ref_prestep_cases as RC
    names = ["edges_two_ranges", "ms_999", "thresh_edges_260", "lead_37"]
    items = [RC.cases()[n] for n in names]
    assert all(rate == 11025 for _, rate, _ in items)
    n_in, ch, cs = [x.shape[0] for x, _, _ in items], [x.shape[1] for x, _, _ in items], [c for _, _, c in items]

    def run(_, t):
        packed, lengths, flags = ops.ref_prestep(t["frames"], n_in, ch, 11025, cs)
        return [packed, torch.tensor(lengths), torch.tensor(flags)]

    _case("ref_prestep", lambda: {"frames": _dev(np.concatenate([x.reshape(-1) for x, _, _ in items]))}, NONE, run)


def _packed_f32(arrays, gap=5, filler=0.123):
    """1-D float32 arrays packed with `gap` filler samples between them -> (host buffer, offsets)"""
    at, offsets = 3, []
    for a in arrays:
        offsets.append(at)
        at += len(a) + gap
    buf = np.full(at, filler, dtype=np.float32)
    for o, a in zip(offsets, arrays):
        buf[o:o + len(a)] = a
    return buf, offsets


DENOISE_CLIPS = (257, 4097, 12000)


def test_ref_denoise_on_a_side_stream():
    clips = [denoise_ref.clip(n) for n in DENOISE_CLIPS]
    buf, off = _packed_f32(clips)
    _case("ref_denoise", lambda: {"wave": _dev(buf)}, NONE, lambda _, t: [ops.ref_denoise(t["wave"], off, [len(c) for c in clips])])


def test_ref_assess_on_a_side_stream():
    clips = [denoise_ref.clip(n) for n in DENOISE_CLIPS]
    raws = [np.clip(3.0 * c, -1.0, 1.0) for c in clips]
    wave, off = _packed_f32(clips)
    raw, raw_off = _packed_f32(raws, gap=37, filler=7.5)
    lens = [len(c) for c in clips]
    _case("ref_assess", lambda: {"raw": _dev(raw), "wave": _dev(wave)}, NONE,
          lambda _, t: [ops.ref_assess(t["raw"], raw_off, [1] * 3, lens, t["wave"], off, lens)])


FLAC_NAMES = ("fixed_2", "lpc_order_8", "stereo_mid_side")


def _flac_tables(names):
    """The host tables `ops.flac_decode_packed` hands f5hip_flac_decode for the named device cases packed back to back"""
    streams = [flac_cases.device_cases()[n]["stream"] for n in names]
    infos = [wave_codec.flac_stream_info(s) for s in streams]
    assert not any(wave_codec.flac_needs_host(f) for f in infos)
    spans, at = [], 0
    for s in streams:
        spans.append((at, at + len(s)))
        at += len(s)
    n = len(names)
    begin = np.array([a + f["first"] for (a, _), f in zip(spans, infos)], dtype=np.int64)
    end = np.array([b for _, b in spans], dtype=np.int64)
    total = np.array([f["total"] for f in infos], dtype=np.int64)
    most = np.array([wave_codec.FLAC_MAX_SECONDS * f["rate"] for f in infos], dtype=np.int64)
    info = np.zeros((n, 8), dtype=np.int32)
    out_off, words = np.zeros(n, dtype=np.int64), 2 * n
    for i, f in enumerate(infos):
        cap = int(_lib.lib().f5hip_flac_decode_bound(int(total[i]), int(end[i] - begin[i]), int(most[i])))
        info[i] = (f["channels"], f["bits"], f["rate"], f["min_block"], f["max_block"], cap, 0, 0)
        out_off[i] = words
        words += int(info[i, 0]) * cap
    return np.frombuffer(b"".join(streams), dtype=np.uint8), begin, end, info, total, most, out_off, words


def _flac_run(tables):
    data_host, begin, end, info, total, most, out_off, words = tables
    n = len(begin)

    def run(_, t):
        """The C entry through ctypes with device pointers (the wrapper uploads the bytes itself); the statuses, the counts and each stream's
        decoded samples: what lies behind a count is never written"""
        out = torch.empty(words, device=DEV, dtype=torch.int32)
        _lib.check(_lib.lib().f5hip_flac_decode(n, _p(t["data"]), t["data"].numel(), _p(begin), _p(end), _p(info), _p(total), _p(most), _p(out), _p(out_off),
                                                _p(out), _lib.current_stream_ptr()), "f5hip_flac_decode")
        head = out[:2 * n].cpu().numpy()
        assert (head[0::2] == 0).all(), head
        parts = [out[:2 * n]]
        for i in range(n):
            ch, cap, count = int(info[i, 0]), int(info[i, 5]), int(head[2 * i + 1])
            parts.append(out[out_off[i]:out_off[i] + ch * cap].view(ch, cap)[:, :count])
        return parts

    return run


def test_flac_decode_on_a_side_stream():
    tables = _flac_tables(FLAC_NAMES)
    _case("flac_decode", lambda: {"data": _dev(tables[0].copy())}, NONE, _flac_run(tables))


def _marked(n, seed, key):
    return wave_codec.mark_pcm16(watermark_ref.host(n, seed), key).astype(np.float32) / np.float32(32768.0)


WM_CLIPS = ((12000, 2, K1), (16385, 4, K2))     # the shortest scored clips of tests/test_gpu_watermark_detect.py


@pytest.mark.parametrize("ids", [False, True], ids=["watermark_detect", "watermark_read_ids"])
def test_watermark_detect_on_a_side_stream(ids):
    buf, off = _packed_f32([_marked(*c) for c in WM_CLIPS])
    carriers = (ops.watermark_tag_carriers if ids else ops.watermark_carriers)([K1, K2], torch.device(DEV))
    call = ops.watermark_read_ids if ids else ops.watermark_detect
    _case(call.__name__, lambda: {"wave": _dev(buf)}, NONE, lambda _, t: [call(t["wave"], off, [c[0] for c in WM_CLIPS], carriers)])


SCAN_N = 2 * wave_codec.WATERMARK_PERIOD + 1000
SCAN_RANGES = [(0, 2), (1, 2), (2, 1), (0, 3)]


@pytest.mark.parametrize("ids", [False, True], ids=["keys", "ids"])
def test_watermark_scan_on_a_side_stream(ids):
    x = _marked(SCAN_N, 11, wave_codec.WatermarkTag(K1, 0x2A5F3C91))
    carriers = (ops.watermark_tag_carriers if ids else ops.watermark_carriers)([K1, K2], torch.device(DEV))
    _case(f"watermark_scan_rows ids={ids}", lambda: {"wave": _dev(x)}, NONE, lambda _, t: [ops.watermark_scan_rows(t["wave"], SCAN_RANGES, carriers, ids=ids)])


# ---------------------------------------------------------------------------------------------------------------- behind the vocoder
FADE = 240
PCM_LENS = (5000, 12345, 801)
PCM_CUTS = (5000, 12000, 801)          # the device-side lengths: request 1 ends below its bound


def _pcm_layout(lens):
    offsets, off = [], 0
    for n in lens:
        offsets.append(off)
        off += (n + 7) & ~7
    return offsets, off + 8


def _pcm_buffer(lens=PCM_LENS, seed=70):
    offsets, total = _pcm_layout(lens)
    buf = np.full(total, 23456, dtype=np.int16)
    for i, (o, n) in enumerate(zip(offsets, lens)):
        buf[o:o + n] = watermark_ref.host(max(n, 2), seed + i)[:n]
    return buf, offsets


def _valid(data, offsets, counts, scale=1):
    """The parts of a packed output that the call writes: request i's counts[i] * scale values at offsets[i]"""
    counts = counts.cpu().tolist()
    return [data[o:o + m * scale] for o, m in zip(offsets, counts)]


def _pcm_case(name, run, binding="default", lens=PCM_LENS, cuts=PCM_CUTS):
    """`run(pcm, offsets, lens, len_dev)` over three requests of ragged lengths in one packed buffer with their device-side lengths"""
    buf, offsets = _pcm_buffer(lens)
    len_dev = torch.tensor(cuts, dtype=torch.int32, device=DEV)      # a length table: there before the delay starts
    torch.cuda.synchronize()
    _case(name, lambda: {"pcm": _dev(buf)}, NONE, lambda _, t: run(t["pcm"], offsets, list(lens), len_dev), binding)


def _finish_inputs():
    w = [_noise(n, 80 + i) for i, n in enumerate((3000, 2000, 36000, 4000, 1500))]
    w[2][6000:33000] = 0.0                                         # a pause of more than a second in the flagged request
    return {f"c{i}": _dev(x) for i, x in enumerate(w)}


def _finish_run(joins):
    def run(_, t):
        chunks = [t[f"c{i}"] for i in range(5)]
        if joins:
            pcm, lengths, offsets = ops.wave_finish_joins(chunks, [2, 2, 1], FADE, [True, False, True, True, True], [False, True, False])
        else:
            pcm, lengths, offsets = ops.wave_finish(chunks, [2, 2, 1], FADE, [False, True, False])
        return [lengths] + _valid(pcm, offsets, lengths)
    return run


@pytest.mark.parametrize("joins", [False, True], ids=["wave_finish", "wave_finish_joins"])
def test_wave_finish_on_a_side_stream(joins):
    _case("wave_finish_joins" if joins else "wave_finish", _finish_inputs, NONE, _finish_run(joins))


def _prosody_run(keep):
    def run(pcm, offsets, lens, len_dev):
        if keep:
            pcm2, len2, off2, _ = ops.wave_prosody(pcm, offsets, lens, len_dev, [(1, 1), (5, 4), (1, 1)], [3, 0, -2], [True, False, False])
        else:
            pcm2, len2, off2, _ = ops.wave_prosody(pcm, offsets, lens, len_dev, [(5, 4), (1, 1), (1, 1)], [0, 3, 0])
        return [len2] + _valid(pcm2, off2, len2)
    return run


@pytest.mark.parametrize("keep", [False, True], ids=["tempo_and_pitch", "keep_formants"])
def test_wave_prosody_on_a_side_stream(keep):
    _pcm_case(f"wave_prosody keep_formants={keep}", _prosody_run(keep))


def _loudness_run(pcm, offsets, lens, len_dev):
    k = wave_codec.loudness_gain_constant
    return [ops.wave_loudness(pcm, offsets, lens, len_dev, [k(-20), None, k(-16)]), pcm]


def test_wave_loudness_on_a_side_stream():
    _pcm_case("wave_loudness", _loudness_run)


def _mark_run(tagged):
    keys = [wave_codec.WatermarkTag(K1, 0x2A5F3C91), None, K2] if tagged else [K1, None, K2]
    return lambda pcm, offsets, lens, len_dev: [ops.wave_mark(pcm, offsets, lens, len_dev, keys)]


@pytest.mark.parametrize("tagged", [False, True], ids=["wave_mark", "wave_mark_ids"])
def test_wave_mark_on_a_side_stream(tagged):
    _pcm_case("wave_mark_ids" if tagged else "wave_mark", _mark_run(tagged))


def _encode_run(rate, enc):
    taps = None if rate == RATE else infer._device_taps(RATE, rate, torch.device(DEV))

    def run(pcm, offsets, lens, len_dev):
        data, out_len, out_off = ops.wave_encode(pcm, offsets, lens, len_dev, rate, enc, taps)
        return [out_len] + _valid(data, out_off, out_len, 2 if enc == "pcm16" else 1)
    return run


@pytest.mark.parametrize("rate,enc", [(8000, "mulaw"), (RATE, "pcm16")], ids=["8000_mulaw", "identity_rate"])
def test_wave_encode_on_a_side_stream(rate, enc):
    _pcm_case(f"wave_encode {rate} {enc}", _encode_run(rate, enc))


def test_wave_encode_on_a_side_stream_through_ctypes():
    _pcm_case("wave_encode 8000 mulaw", _encode_run(8000, "mulaw"), "ctypes")


def _flac_out_run(level):
    def run(pcm, offsets, lens, len_dev):
        data, out_len, out_off = ops.wave_flac(pcm, offsets, lens, len_dev, RATE, level)
        return [out_len] + _valid(data, out_off, out_len)
    return run


@pytest.mark.parametrize("level", [None, [1, 0, 1]], ids=["level_0", "level_1"])
def test_wave_flac_on_a_side_stream(level):
    _pcm_case(f"wave_flac level {level}", _flac_out_run(level))


# ---------------------------------------------------------------------------------------------------------------- one chain
def test_the_delivery_chain_on_a_side_stream():
    """`infer.finish_requests(..., device_backend=True)` over four requests that between them use every stage -- silence removal, tempo,
    pitch with and without its formants, a mark with and without a trace id, a loudness target, G.711, a resampled FLAC at level 1 -- on
    the side stream vs the same call on the default stream: the bytes and `backend_stats`."""
    opts = dict(sample_rate=[None, 8000, 16000, 24000], encoding=[None, "mulaw", "flac", "flac"], loudness=[None, -20, None, -16], flac_level=[None, None, 1, 0],
                tempo=[None, 1.25, None, None], pitch=[None, None, 3, -2], watermark=[None, K1, wave_codec.WatermarkTag(K2, 77), None],
                keep_formants=[None, None, None, True])
    silence = [True, False, False, False]
    sizes = [(36000, 12000), (12000, 9000), (12000,), (9000, 12000)]
    stats = []

    def inputs():
        t, k = {}, 0
        for r, req in enumerate(sizes):
            for c, n in enumerate(req):
                w = _noise(n, 90 + k)
                if (r, c) == (0, 0):
                    w[6000:33000] = 0.0
                t[f"r{r}c{c}"] = _dev(w)
                k += 1
        return t

    def run(_, t):
        waves = [[t[f"r{r}c{c}"] for c in range(len(req))] for r, req in enumerate(sizes)]
        infer.backend_stats.clear()
        out = infer.finish_requests(waves, [""] * 4, infer.cross_fade_duration, silence, device_backend=True, want="pcm16", **opts)
        stats.append(dict(infer.backend_stats))
        return [torch.from_numpy(np.frombuffer(o.tobytes(), dtype=np.uint8).copy()) for o in out]

    H.same_bits_on_a_side_stream("finish_requests chain", inputs, NONE, run)
    print("[streams] finish_requests chain backend_stats:", sorted(stats[0].items()))
    assert stats[0].get("host_requests", 0) == 0 and stats[0]["device_requests"] == 4
    assert all(s == stats[0] for s in stats), stats


# ---------------------------------------------------------------------------------------------------------------- part 3: two streams
def _two_streams(name, a_inputs, a_run, b_inputs, b_run, a_pending=True):
    """Call A on stream s1 behind the late producer, call B at once on stream s2 with its own buffers; then both streams are synchronised.
    A's outputs equal A alone on the default stream bit for bit, B's equal B alone.  B's data inputs are complete before it is issued: it
    has no reason of its own to wait.  `a_pending`: A returns without a host wait, so its producer has still not run when B is issued
    (asserted); an `upload_sync` entry waits on the host for its upload, and with it for the producer, before it launches: there only
    A's launches can still be pending, and nothing can be asserted about them."""
    want_a, real_a, host_ms = H.default_stream_run(name + " A", a_inputs, NONE, a_run)
    want_b, real_b, _ = H.default_stream_run(name + " B", b_inputs, NONE, b_run)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s2):
        bufs_b = {k: v.clone() for k, v in real_b.items()}
    s2.synchronize()
    with torch.cuda.stream(s1):
        bufs = {k: H.poison_like(v) for k, v in real_a.items()}
        s1.synchronize()
        e0, e1 = H.queue_delay(s1, max(H.DELAY_FACTOR * host_ms, H.MIN_DELAY_MS))
        for k, v in real_a.items():
            bufs[k].copy_(v)
        produced = torch.cuda.Event()
        produced.record(s1)
        assert not produced.query()
        out_a = a_run(None, bufs)
        got_a = [o.clone() for o in out_a]
    if a_pending:
        assert not produced.query(), f"{name}: A was no longer pending when B was issued"
    with torch.cuda.stream(s2):
        got_b = [o.clone() for o in b_run(None, bufs_b)]
    s1.synchronize()
    s2.synchronize()
    print(f"[streams] {name}: two streams, A behind a delay of {e0.elapsed_time(e1):.1f} ms (host {host_ms:.3f} ms)")
    H.same(got_a, want_a, f"{name}: A on stream 1 with B behind it on stream 2 vs A alone")
    H.same(got_b, want_b, f"{name}: B on stream 2 behind A on stream 1 vs B alone")


B_LENS, B_CUTS = (2400, 801), (2400, 700)


def _pcm_pair(name, a_run, b_run, a_pending=True):
    """A: the three requests of part 1; B: two requests, each offset + length inside A's extents"""
    a_buf, a_off = _pcm_buffer(PCM_LENS)
    b_buf, b_off = _pcm_buffer(B_LENS, seed=75)
    assert len(B_LENS) < len(PCM_LENS) and all(o + n <= a_off[-1] + PCM_LENS[-1] for o, n in zip(b_off, B_LENS)) and len(b_buf) <= len(a_buf)
    assert all(n <= m for n, m in zip(B_LENS, PCM_LENS))
    a_len = torch.tensor(PCM_CUTS, dtype=torch.int32, device=DEV)
    b_len = torch.tensor(B_CUTS, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    _two_streams(name, lambda: {"pcm": _dev(a_buf)}, lambda _, t: a_run(t["pcm"], a_off, list(PCM_LENS), a_len),
                 lambda: {"pcm": _dev(b_buf)}, lambda _, t: b_run(t["pcm"], b_off, list(B_LENS), b_len), a_pending)


@pytest.mark.parametrize("tagged", [False, True], ids=["wave_mark", "wave_mark_ids"])
def test_two_streams_wave_mark(tagged):
    """B's keys are among A's (key rows 0 and 1 of two)"""
    keys = [wave_codec.WatermarkTag(K2, 5), K1] if tagged else [K2, K1]
    _pcm_pair("wave_mark_ids" if tagged else "wave_mark", _mark_run(tagged),
              lambda pcm, offsets, lens, len_dev: [ops.wave_mark(pcm, offsets, lens, len_dev, keys)])


def _f32_pair(name, sizes_a, sizes_b, make, call):
    """A over the clips `sizes_a`, B over fewer and no longer clips `sizes_b`, each in its own packed buffer"""
    assert len(sizes_b) < len(sizes_a) and all(b <= a for a, b in zip(sizes_a, sizes_b))
    bufs = []
    for sizes, seed in ((sizes_a, 0), (sizes_b, 100)):
        clips = [make(n, seed + i) for i, n in enumerate(sizes)]
        buf, off = _packed_f32(clips)
        bufs.append((buf, off, list(sizes)))
    assert all(o + n <= bufs[0][1][-1] + sizes_a[-1] for o, n in zip(bufs[1][1], sizes_b))
    (a, ao, an), (b, bo, bn) = bufs
    _two_streams(name, lambda: {"wave": _dev(a)}, lambda _, t: [call(t["wave"], ao, an)], lambda: {"wave": _dev(b)}, lambda _, t: [call(t["wave"], bo, bn)])


def test_two_streams_ref_denoise():
    _f32_pair("ref_denoise", DENOISE_CLIPS, (257, 1024), lambda n, s: denoise_ref.clip(n), ops.ref_denoise)


def test_two_streams_ref_assess():
    def call(wave, off, lens):
        return ops.ref_assess(wave, off, [1] * len(lens), lens, wave, off, lens)     # (the prepared clips stand in for the raw ones)
    _f32_pair("ref_assess", DENOISE_CLIPS, (257, 1024), lambda n, s: denoise_ref.clip(n), call)


@pytest.mark.parametrize("ids", [False, True], ids=["watermark_detect", "watermark_read_ids"])
def test_two_streams_watermark_detect(ids):
    """A and B score against the same carriers (B's key rows are A's)"""
    carriers = (ops.watermark_tag_carriers if ids else ops.watermark_carriers)([K1, K2], torch.device(DEV))
    call = ops.watermark_read_ids if ids else ops.watermark_detect
    _f32_pair(call.__name__, (16385, 12000, 12000), (12000, 12000), lambda n, s: _marked(n, s, K1 if s % 2 else K2),
              lambda wave, off, lens: call(wave, off, lens, carriers))


def test_two_streams_watermark_scan():
    """B: a shorter recording and fewer ranges, all of them ranges of A's call too"""
    carriers = ops.watermark_carriers([K1, K2], torch.device(DEV))
    a, b = _marked(SCAN_N, 11, K1), _marked(SCAN_N - 1000, 12, K2)
    ranges_b = [(0, 2), (1, 1)]
    assert len(b) <= len(a) and len(ranges_b) < len(SCAN_RANGES) and all(f + c <= 2 for f, c in ranges_b)
    _two_streams("watermark_scan", lambda: {"wave": _dev(a)}, lambda _, t: [ops.watermark_scan_rows(t["wave"], SCAN_RANGES, carriers)],
                 lambda: {"wave": _dev(b)}, lambda _, t: [ops.watermark_scan_rows(t["wave"], ranges_b, carriers)])


def test_two_streams_ref_prestep():
    """Through ctypes: `ops.ref_prestep` downloads the lengths, which would wait for A.  The output is zeroed on the call's stream first,
    so what lies behind a clip's kept samples is the same in every run."""
    import ref_prestep_cases as RC

    def pack(names):
        items = [RC.cases()[n] for n in names]
        frames = np.concatenate([x.reshape(-1) for x, _, _ in items])
        ni, ch = (np.array([x.shape[d] for x, _, _ in items], dtype=np.int32) for d in (0, 1))
        cs = np.array([c for _, _, c in items], dtype=np.uint8)
        bound = int(_lib.lib().f5hip_ref_prestep_bound(len(ni), _p(ni), _p(ch), 11025))

        def run(_, t):
            out, info = torch.zeros(bound, device=DEV), torch.zeros(len(ni), 2, device=DEV, dtype=torch.int32)
            _lib.check(_lib.lib().f5hip_ref_prestep(len(ni), _p(ni), _p(ch), _p(cs), _p(t["frames"]), t["frames"].numel(), 11025, _p(out), _p(info),
                                                    _lib.current_stream_ptr()), "f5hip_ref_prestep")
            return [out, info]
        return frames, ni.tolist(), run
    fa, na, run_a = pack(["edges_two_ranges", "ms_999", "thresh_edges_260", "lead_37"])
    fb, nb, run_b = pack(["lead_37", "ms_99"])
    assert len(nb) < len(na) and len(fb) <= len(fa) and max(nb) <= max(na)
    _two_streams("ref_prestep", lambda: {"frames": _dev(fa)}, run_a, lambda: {"frames": _dev(fb)}, run_b)


def test_two_streams_wave_encode():
    """An `upload_sync` entry: the second call's upload waits on the host for its own stream only, and the first call's kernel is queued
    behind a delay, so the window is there -- but it is one launch wide.  A regression net, not a proof."""
    _pcm_pair("wave_encode", _encode_run(8000, "mulaw"), _encode_run(8000, "mulaw"), a_pending=False)


def test_two_streams_mel_ragged():
    """The other `upload_sync` entry, with the same reservation: a regression net, not a proof."""
    a, b = CLIPS, (1024, 4411)
    assert len(b) < len(a) and all(y <= x for x, y in zip(a, b))
    _two_streams("mel_spectrogram_ragged", lambda: {f"w{i}": _dev(_noise(n, 52 + i)) for i, n in enumerate(a)},
                 lambda _, t: [mel_spectrogram_ragged([t[f"w{i}"] for i in range(len(a))], "vocos")[0]],
                 lambda: {f"w{i}": _dev(_noise(n, 152 + i)) for i, n in enumerate(b)},
                 lambda _, t: [mel_spectrogram_ragged([t[f"w{i}"] for i in range(len(b))], "vocos")[0]], a_pending=False)
