"""FLAC level 1 on the device (csrc/wave_out.h wave_flac_frame_kernel<true>, f5hip_wave_flac_levels: LPC subframes among the candidates of
the full blocks of the requests that ask for them) against the host definition `wave_codec.encode_flac(x, rate, level)`: ragged batches
with both levels in one call, the level-0 call unchanged, the device decoder on the level-1 streams, and a micro-batch of mixed formats
and levels through `infer_requests` with the device back-end on a tiny model.

Every comparison is equality of bytes and lengths: there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flac_lpc_ref as R  # noqa: E402
from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth, torch_ops, wave_codec as W  # noqa: E402

from test_gpu_request_knobs import ARCH, REF_TEXT, TEXT, VOCAB, _prompt  # noqa: E402
from test_gpu_wave_flac import _check, _counter, _reset  # noqa: E402

LENGTHS = (0, 13, 4096, 4097, 8192 + 5)
RATES = (8000, 24000, 44100)


@pytest.fixture(scope="module")
def matrix():
    """The signal matrix at the five lengths, dealt into batches of 1 to 5 requests: [(pcm, level)] per batch, levels alternating so that
    every batch but the first mixes both; and the frames of the host definition's stream of every request (24 kHz), computed once."""
    sig = R.signals()
    requests = [(x[:n], (i + j) % 2) for i, (name, x) in enumerate(sig.items()) for j, n in enumerate(LENGTHS)]
    requests[0] = (requests[0][0], 1)
    batches, at, size = [], 0, 1
    while at < len(requests):
        batches.append(requests[at:at + size])
        at += size
        size = size % 5 + 1
    want = {}
    for b, batch in enumerate(batches):
        for i, (x, lv) in enumerate(batch):
            frames = W.encode_flac(x, 24000, lv).tobytes()[42:]                      # (the frames differ between rates in one header nibble alone,
            want[(b, i)] = frames                                                     #  so the other rates are encoded for a few batches only)
    return batches, want


def _device(batch, rate, levels="own", cut=None, reverse=False):
    """ops.wave_flac on ONE packed buffer with a loud filler between the requests -> [bytes per request]."""
    dev = torch.device("cuda:0")
    order = list(range(len(batch)))[::-1] if reverse else list(range(len(batch)))
    pcms = [batch[i][0] for i in order]
    level = [batch[i][1] for i in order] if levels == "own" else levels
    offsets, off = [], 0
    for x in pcms:
        offsets.append(off)
        off += (len(x) + 7) & ~7
    buf = np.full(off + 8, 23456, dtype=np.int16)
    for o, x in zip(offsets, pcms):
        buf[o:o + len(x)] = x
    len_dev = None if cut is None else torch.tensor([cut[i] for i in order], dtype=torch.int32, device=dev)
    data, out_len, out_off = ops.wave_flac(torch.from_numpy(buf).to(dev), offsets, [len(x) for x in pcms], len_dev, rate, level=level)
    host, counts = data.cpu().numpy(), out_len.cpu().tolist()
    got = [host[o:o + m].tobytes() for o, m in zip(out_off, counts)]
    return [got[order.index(i)] for i in range(len(batch))]


@pytest.mark.parametrize("rate", RATES)
def test_mixed_levels_equal_the_host_definition_byte_for_byte(matrix, rate):
    batches, want = matrix
    for b, batch in enumerate(batches):
        got = _device(batch, rate)
        for i, (x, lv) in enumerate(batch):
            if rate == 24000:
                _check(got[i][42:], want[(b, i)], (b, i, lv, len(x)))
            if rate != 24000 or b % 4 == 0:
                _check(got[i], W.encode_flac(x, rate, lv).tobytes(), (rate, b, i, lv, len(x)))
            elif len(x):
                assert len(got[i]) == 42 + len(want[(b, i)])


def test_twice_reversed_and_through_both_bindings(matrix):
    batches, _ = matrix
    picks = [batch for batch in batches if len(batch) == 5][:3]
    first = [_device(batch, 44100) for batch in picks]
    assert [_device(batch, 44100) for batch in picks] == first
    assert [_device(batch, 44100, reverse=True) for batch in picks] == first
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        assert [_device(batch, 44100) for batch in picks] == first
    finally:
        torch_ops._loaded = True
    for batch, got in zip(picks, first):
        for (x, lv), g in zip(batch, got):
            _check(g, W.encode_flac(x, 44100, lv).tobytes(), (lv, len(x)))


def test_device_side_lengths_shorter_than_the_bounds(matrix):
    sig = R.signals()
    batch = [(sig["resonance"], 1), (sig["square"], 1), (sig["sine041"], 0), (sig["edges"], 1), (sig["walk"], 1)]
    cut = [4096 + 7, 4096, 8192, 0, 4095]
    got = _device(batch, 8000, cut=cut)
    for i, ((x, lv), n) in enumerate(zip(batch, cut)):
        _check(got[i], W.encode_flac(x[:n], 8000, lv).tobytes(), (i, n))


def test_forty_frames_of_the_resonance():
    """One contraction or one slip in a reduction order anywhere in the recursion changes a coefficient in some frame of forty."""
    x = R.resonance(40 * 4096 + 100, seed=11)
    got, = _device([(x, 1)], 24000)
    want = W.encode_flac(x, 24000, 1)
    _check(got, want.tobytes(), "40 frames")
    kinds = [name for name, _ in R.frames_of(want)]
    assert sum(k.startswith("lpc") for k in kinds) >= 30, kinds                                   # (the frames are LPC subframes: the recursion ran)


def test_level_zero_is_the_old_call(matrix):
    """`level=None` and all-zero levels: the bytes of `encode_flac(x, rate)`, three launches, the counters as before."""
    batches, _ = matrix
    batch = next(b for b in batches if len(b) == 4)
    want = [W.encode_flac(x, 24000).tobytes() for x, _ in batch]
    _device(batch, 24000, levels=None)                                                # (the first call of a process also allocates)
    for levels in (None, 0, [0] * len(batch)):
        _reset()
        got = _device(batch, 24000, levels=levels)
        assert got == want
        assert _counter("wave_flac_launches") == 3 and _counter("wave_flac_requests") == len(batch)
    _reset()
    _device(batch, 24000)                                                             # mixed levels: three launches too
    assert _counter("wave_flac_launches") == 3 and _counter("wave_flac_requests") == len(batch)


def test_refused_levels_launch_nothing():
    pcm = torch.zeros(4096, device="cuda:0", dtype=torch.int16)
    _reset()
    for bad in (2, -1, True, "1", [0, 1], [2]):
        with pytest.raises(_lib.F5HipError, match="level"):
            ops.wave_flac(pcm, [0], [4096], None, 24000, level=bad)
    with pytest.raises(RuntimeError, match="level"):
        torch.ops.f5hip.wave_flac_levels([pcm], torch.zeros(1, dtype=torch.int64), torch.tensor([100], dtype=torch.int32), None, 24000,
                                         torch.tensor([2], dtype=torch.int32))
    assert _counter("wave_flac_launches") == 0 and _counter("wave_flac_requests") == 0


def test_device_decoder_reads_the_level_one_streams():
    sig = R.signals()
    batch = [(sig[name], 1) for name in ("square", "sine041", "resonance", "edges", "smooth_loud_head")]
    streams = _device(batch, 24000)
    assert all(any(name.startswith("lpc") for name, _ in R.frames_of(s)) for s in streams[:4])
    for (x, _), (samples, rate, bits) in zip(batch, ops.flac_decode(streams)):
        assert (rate, bits) == (24000, 16) and np.array_equal(np.asarray(samples).reshape(-1), x)


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def test_infer_requests_mixed_formats_and_levels_in_one_micro_batch(hip_objects, tmp_path):
    """pcm16, mu-law, flac level 0 and flac level 1 requests at two rates in ONE micro-batch with the device back-end: each body is the host
    path's, and the flac requests of a rate share one `ops.wave_flac` call whatever their levels."""
    path = _prompt(tmp_path)
    text = TEXT[:110]
    opts = [dict(seed=7), dict(seed=7, sample_rate=8000, encoding="mulaw"), dict(seed=7, encoding="flac"), dict(seed=7, encoding="flac", flac_level=1),
            dict(seed=7, encoding="flac", sample_rate=8000, flac_level=1), dict(seed=7, encoding="flac", sample_rate=8000, flac_level=0)]
    out = {}
    for backend in (True, False):
        mgr = serve.TTSManager(nfe_step=8, device_backend=backend).load(*hip_objects)
        try:
            voice, ref_text_n = mgr._voice(path, REF_TEXT)
            batch = [(voice, ref_text_n, text, o) for o in opts]
            _reset()
            infer.backend_stats.clear()
            out[backend] = mgr._run_batch(batch)
            if backend:
                assert infer.backend_stats["device_requests"] == len(batch) and infer.backend_stats.get("host_requests", 0) == 0
                assert infer.backend_stats["flac_calls"] == 2 and infer.backend_stats["flac_requests"] == 4      # one call per distinct rate
                assert _counter("wave_flac_requests") == 4 and _counter("wave_flac_launches") == 6
            else:
                assert _counter("wave_flac_launches") == 0
        finally:
            mgr.close()
    dev, host = out[True], out[False]
    pcm = dev[0]
    assert pcm.dtype == np.int16 and np.array_equal(dev[1], infer.deliver_pcm16(pcm, 8000, "mulaw"))
    for i in range(2, 6):
        assert dev[i].dtype == host[i].dtype == np.uint8 and dev[i].tobytes() == host[i].tobytes(), i
        rate, level = opts[i].get("sample_rate", 24000), opts[i].get("flac_level", 0)
        assert dev[i].tobytes() == infer.deliver_pcm16(pcm, rate, "flac", level if level else None).tobytes(), i
        y, r, _ = W.read_flac(dev[i].tobytes())
        assert r == rate and np.array_equal(y[0], infer.resample_pcm16(pcm, rate)), i
    assert len(dev[3]) <= len(dev[2]) and len(dev[4]) <= len(dev[5])


def test_a_streamed_level_one_request_has_the_whole_ones_frames(hip_objects, tmp_path):
    path, text = _prompt(tmp_path), TEXT[:110]
    mgr = serve.TTSManager(nfe_step=8, micro_batch=dict(span_steps=3), device_backend=True).load(*hip_objects)
    try:
        _reset()
        pcm = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, seed=7)
        whole = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, seed=7, encoding="flac", sample_rate=8000, flac_level=1)
        assert whole.dtype == np.uint8 and whole.tobytes() == infer.deliver_pcm16(pcm, 8000, "flac", 1).tobytes()
        assert _counter("wave_flac_requests") == 1
        pieces = list(mgr.synthesize_stream(text, ref_audio_path=path, ref_text=REF_TEXT, seed=7, encoding="flac", sample_rate=8000, flac_level=1))
        assert pieces[0].tobytes() == infer.StreamFlacEncoder(8000, 1).header()
        assert np.concatenate(pieces).tobytes()[42:] == whole.tobytes()[42:]
    finally:
        mgr.close()
