"""The true-peak limiter on the device (csrc/wave_limit.h, f5hip_wave_loudness_limit: the 24 kHz int16 PCM of a ragged batch of requests, in
place, number, tag and plain requests together in four launches) against the host definition `wave_codec.limit_pcm16`, alone and through
`TTSManager(device_backend=True)` on a tiny model.

Every comparison is equality of bytes: there is no tolerance anywhere."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import infer, ops, serve, torch_ops, wave_codec  # noqa: E402
from tts_indic_server_f5_amd.wave_codec import LoudnessTag as Tag  # noqa: E402

from test_gpu_request_knobs import REF_TEXT, TEXT, _prompt  # noqa: E402
from test_gpu_wave_mark import FILLER, _compare, _counter, _reset, hip_objects  # noqa: E402,F401
from test_loudness_host import _bursts, _sine  # noqa: E402

M, T = wave_codec.LIMIT_HOLD, 2048                      # f5hip_wave_loudness_limit_tile(): checked below
LENGTHS = (0, 1, 6, 7, M, M + 1, 2 * M + 1, T - 1, T, T + 1, 2 * T + 3, 30011)
KINDS = ("zeros", "square", "sine", "click first", "click last", "burst", "speech")
OPTIONS = (Tag(None, -1.0), Tag(-16.0, -1.0), -20.0, Tag(-10.0, -3.0), None, Tag(None, -3.0))


def _content(kind, n, seed):
    x = np.zeros(n, dtype=np.int16)
    if kind == "square":
        x[0::2], x[1::2] = 32767, -32768
    elif kind == "sine":                                # peaks between the samples only
        x = _sine(n, 6000, -0.5, math.pi / 4)
    elif kind == "click first" and n:
        x[0] = -32768
    elif kind == "click last" and n:
        x[-1] = 32767
    elif kind == "burst" and n >= 8:
        x[n // 3:n // 3 + n // 8] = _bursts(n // 8, seed, -3.0)
    elif kind == "speech" and n:
        x = _bursts(n, seed, -18.0)
    elif kind.startswith("click at"):                   # a quiet host (so that the fast tiles have a gain to apply) with one click
        x = _bursts(n, seed, -45.0)
        x[int(kind.split()[-1])] = 32767
    return np.ascontiguousarray(x)


def _requests():
    """(samples, option, device length or None): every length with every content, the options in rotation; three clicks around a tile
    boundary in 5-tile requests, so that slow tiles border fast ones on both sides; device lengths below the bounds."""
    out = [(_content(kind, n, 7 * i + j), OPTIONS[(i + j) % len(OPTIONS)], None) for i, n in enumerate(LENGTHS) for j, kind in enumerate(KINDS)]
    out += [(_content(f"click at {at}", 5 * T + 3, at), Tag(-20.0, -2.0), None) for at in (2 * T - M, 2 * T, 2 * T + M)]
    out += [(_content("speech", 30011, 99), Tag(-12.0, -1.0), 20000), (_content("square", 2 * T + 3, 0), Tag(None, -1.0), T + 1),
            (_content("speech", 30011, 98), -16.0, 25001), (_content("sine", 9000, 0), None, 100)]
    return out


def _device(requests):
    """ops.wave_loudness(..., true_peak=) on ONE packed buffer with the requests at `wave_finish`'s 8-sample offsets and a loud filler
    between them -> (the whole buffer afterwards, the buffer before, its offsets, the stats rows)."""
    dev = torch.device("cuda:0")
    offsets, off = [], 0
    for x, _, _ in requests:
        offsets.append(off)
        off += (len(x) + 7) & ~7
    buf = np.full(off + 8, FILLER, dtype=np.int16)
    for o, (x, _, _) in zip(offsets, requests):
        buf[o:o + len(x)] = x
    pcm = torch.from_numpy(buf.copy()).to(dev)
    specs = [infer.WaveSpec(loudness=option) for _, option, _ in requests]
    cuts = [len(x) if cut is None else cut for x, _, cut in requests]
    len_dev = None if all(cut is None for _, _, cut in requests) else torch.tensor(cuts, dtype=torch.int32, device=dev)
    stats = ops.wave_loudness(pcm, offsets, [len(x) for x, _, _ in requests], len_dev, [s.gain_constant for s in specs], true_peak=[s.ceiling for s in specs])
    return pcm.cpu().numpy(), buf, offsets, stats.cpu().numpy()


@pytest.fixture(scope="module")
def batch_run():
    requests = _requests()
    _reset()
    return (requests,) + _device(requests) + ((_counter("wave_limit_launches"), _counter("wave_limit_requests"), _counter("wave_loudness_launches")),)


def test_ragged_batch_equals_the_host_definition_bit_for_bit(batch_run):
    """A tag request's bytes are `limit_pcm16`'s and a number request's `normalise_loudness_pcm16`'s; the sentinel gaps, the plain requests
    and the samples past a device length keep their bits; a request with a target has the meter's stats row; four launches."""
    assert ops.wave_loudness_limit_tile() == T and ops.wave_loudness_limit_launches() == 4
    requests, got, buf, offsets, stats, counters = batch_run
    want, rows = buf.copy(), np.zeros_like(stats)
    for i, (o, (x, option, cut)) in enumerate(zip(offsets, requests)):
        n = len(x) if cut is None else cut
        want[o:o + n] = wave_codec.limit_pcm16(x[:n], option)
        target = option.target if isinstance(option, Tag) else option
        if target is not None:
            n2, S2, peak = infer.measure_loudness(x[:n])
            g = infer.loudness_gain(n2, S2, peak, infer.loudness_gain_constant(target))
            rows[i] = (n2, S2, peak, np.float64(g).view(np.int64))
    _compare(got, want, "batch")
    assert np.array_equal(stats, rows)
    assert counters == (4, sum(isinstance(option, Tag) for _, option, _ in requests), 0)
    acted = [isinstance(option, Tag) and not np.array_equal(got[o:o + len(x)], infer.normalise_loudness_pcm16(x, option.target))
             for o, (x, option, _) in zip(offsets, requests)]
    assert sum(acted) > 20 and all(acted[-7:-4])                                         # the limiter acts, in the boundary clicks too


def test_each_request_equals_its_single_request_call_and_the_reversed_batch(batch_run):
    requests, got, _, offsets, stats, _ = batch_run
    for i, (o, (x, option, _)) in enumerate(zip(offsets, requests)):
        if option is not None:
            solo, _, _, row = _device([requests[i]])
            assert np.array_equal(solo[:len(x)], got[o:o + len(x)]) and np.array_equal(row[0], stats[i]), i
    back, _, boff, brows = _device(requests[::-1])
    for i, (o, (x, _, _)) in enumerate(zip(offsets, requests)):
        j = len(requests) - 1 - i
        assert np.array_equal(back[boff[j]:boff[j] + len(x)], got[o:o + len(x)]) and np.array_equal(brows[j], stats[i]), i


def test_ctypes_and_torch_op_paths_agree(batch_run):
    requests, got, _, _, stats, _ = batch_run
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again, _, _, rows = _device(requests)
    finally:
        torch_ops._loaded = True
    assert np.array_equal(got, again) and np.array_equal(stats, rows)


def test_a_call_without_a_ceiling_is_wave_loudness(batch_run):
    """Numbers only: `true_peak` all None gives `ops.wave_loudness`'s bytes, stats and counters, and none of the limiter's."""
    requests = [(x, option.target if isinstance(option, Tag) else option, cut) for x, option, cut in batch_run[0]]
    _reset()
    got, buf, offsets, stats = _device(requests)
    counters = (_counter("wave_loudness_launches"), _counter("wave_loudness_requests"), _counter("wave_limit_launches"))
    assert counters == (3, sum(option is not None for _, option, _ in requests), 0)
    pcm = torch.from_numpy(buf.copy()).to("cuda:0")
    cuts = torch.tensor([len(x) if cut is None else cut for x, _, cut in requests], dtype=torch.int32, device="cuda:0")
    rows = ops.wave_loudness(pcm, offsets, [len(x) for x, _, _ in requests], cuts, [infer.WaveSpec(loudness=o).gain_constant for _, o, _ in requests])
    assert np.array_equal(pcm.cpu().numpy(), got) and np.array_equal(rows.cpu().numpy(), stats)
    with pytest.raises(Exception, match="ceiling"):
        ops.wave_loudness(pcm, offsets[:1], [100], None, [None], true_peak=[5])
    assert np.array_equal(pcm.cpu().numpy(), got)


def test_manager_micro_batch_with_a_tag_a_number_and_a_plain_request(hip_objects, tmp_path):  # noqa: F811
    """Through `TTSManager(device_backend=True)`: the three in ONE micro-batch equal the host back-end (`finish_pcm16`) byte for byte, in
    one `ops.wave_loudness` call, with the device-to-host copies of the same batch with a number in the tag's place."""
    path = _prompt(tmp_path)
    tag = {"target": -14.0, "true_peak": -2.0}
    out, copies = {}, {}
    for backend, option in ((True, tag), (False, tag), (True, -14.0)):
        mgr = serve.TTSManager(nfe_step=8, device_backend=backend).load(*hip_objects)
        try:
            voice, ref_text_n = mgr._voice(path, REF_TEXT)
            batch = [(voice, ref_text_n, TEXT[:110], o) for o in (dict(seed=7, loudness=option), dict(seed=7, loudness=-20.0), dict(seed=7))]
            _reset()
            infer.backend_stats.clear()
            out[backend, option is tag] = mgr._run_batch(batch)
            copies[backend, option is tag] = infer.backend_stats["d2h_copies"]
            if backend:
                assert infer.backend_stats["device_requests"] == 3 and infer.backend_stats["loudness_calls"] == 1
                assert infer.backend_stats["limit_requests"] == (option is tag) == (_counter("wave_limit_launches") == 4)
        finally:
            mgr.close()
    assert copies[True, True] == copies[True, False]
    for d, h in zip(out[True, True], out[False, True]):
        h = h if h.dtype != np.float32 else infer.quantise_pcm16(h)                     # (the host back-end leaves a request without options as float32)
        assert d.dtype == h.dtype and np.array_equal(d, h)
    plain = out[True, True][2]
    assert np.array_equal(out[True, True][0], wave_codec.limit_pcm16(plain, tag)) and not np.array_equal(out[True, True][0], out[True, False][0])
    assert np.array_equal(out[True, True][1], out[True, False][1]) and np.array_equal(plain, out[True, False][2])
