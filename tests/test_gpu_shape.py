"""The formant shift on the device (csrc/wave_formant.h wave_shape_kernel, f5hip_wave_prosody_shape: `ops.wave_prosody(..., formant=)`)
against the host definition `infer.shift_pcm16(pcm, tempo, PitchTag(s, f))`.  Every comparison is equality of bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, torch_ops  # noqa: E402

from test_formant_host import LENGTHS, content, vowel  # noqa: E402
from test_gpu_formant import FILLER, _compare, _counter, _reset  # noqa: E402

Tag = infer.PitchTag
KINDS = ("zeros", "noise", "vowel", "mixed")
# (tempo, pitch, keep_formants) per request: the issue's six moves, a shaped request with its flag set, plain and kept ones
OPTIONS = [(1.0, Tag(0, 1), False), (0.8, Tag(0, -6), False), (1.25, Tag(0, 6), False), (1.0, Tag(3, -3), False), (0.8, Tag(-2, 4), True), (1.0, 6, True),
           (1.25, 2, False), (1.0, 0, False), (1.25, -4, True)]


def _device(batch):
    """`ops.wave_prosody(..., formant=)` on one packed buffer, a loud filler between the requests -> each request's samples."""
    offsets = np.cumsum([0] + [(len(x) + 7 & ~7) + 8 for x, _ in batch]).tolist()
    buf = np.full(offsets[-1], FILLER, dtype=np.int16)
    for o, (x, _) in zip(offsets, batch):
        buf[o:o + len(x)] = x
    pcm, specs = torch.from_numpy(buf.copy()).to("cuda:0"), [infer.WaveSpec(tempo=t, pitch=p, keep_formants=k) for _, (t, p, k) in batch]
    pcm2, len2, off2, _ = ops.wave_prosody(pcm, offsets[:-1], [len(x) for x, _ in batch], None, [s.stretch for s in specs], [s.semitones for s in specs],
                                           keep_formants=[s.keep_formants for s in specs], formant=[s.formant for s in specs])
    host = pcm2.cpu().numpy()
    assert np.array_equal(pcm.cpu().numpy(), buf)                                          # the input, filler included, is not written
    return [host[o:o + m].copy() for o, m in zip(off2, len2.cpu().tolist())]


@pytest.mark.parametrize("turn", range(4))
def test_the_kernel_equals_the_host_definition_bit_for_bit(turn):
    """The 7 lengths in ragged batches of 3 and 4; over the turns every length meets every content, and the options rotate past them."""
    cases = [(content(KINDS[(j + turn) % 4], n), OPTIONS[(j + 2 * turn) % len(OPTIONS)]) for j, n in enumerate(LENGTHS)]
    for batch in (cases[:3], cases[3:]):
        for g, (x, (t, p, k)) in zip(_device(batch), batch):
            _compare(g, infer.shift_pcm16(x, t, p, keep_formants=k), (turn, len(x), t, p, k))


def test_a_request_does_not_depend_on_its_call_and_both_bindings_agree():
    batch = [(content(k, n), o) for k, n, o in zip(("vowel", "mixed", "mixed", "vowel"), (30011, 24000, 1000, 20000), OPTIONS[1:5])]
    got, back = _device(batch), _device(batch[::-1])
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        again = _device(batch)
    finally:
        torch_ops._loaded = True
    for i in range(len(batch)):
        assert all(np.array_equal(v, got[i]) for v in (_device(batch[i:i + 1])[0], back[-1 - i], again[i])), i


def test_launch_counts_and_refusals_before_any_launch():
    """A shaped request: WSOLA + 3 (the resampler beside a plain pitch).  No step in the call: today's counts.  A call the library or the
    operator refuses launches nothing and leaves the output and its lengths as they were."""
    x = vowel(5000, 130)
    _device([(x, OPTIONS[3])])                                                             # (the first call of a process also allocates)
    for opts, want in (([OPTIONS[3], OPTIONS[5], OPTIONS[7]], (1, 3, 2)), ([OPTIONS[3], OPTIONS[6]], (2, 3, 1)), ([OPTIONS[5], OPTIONS[6]], (2, 3, 1))):
        _reset()
        _device([(x, o) for o in opts])
        assert (_counter("wave_prosody_launches"), _counter("wave_formant_launches"), _counter("wave_formant_requests")) == want, opts
    lib, dev = _lib.lib(), torch.device("cuda:0")
    pcm, out, lens = torch.from_numpy(x).to(dev), torch.full((8192,), 77, device=dev, dtype=torch.int16), torch.full((1,), -5, device=dev, dtype=torch.int32)
    i32 = lambda v: np.asarray([v], dtype=np.int32)   # noqa: E731
    t32 = lambda v: torch.tensor([v], dtype=torch.int32)   # noqa: E731
    _reset()
    for pitch, step, text in ((3, None, "bad argument"), (0, 7, "formant step of 7 semitones"), (3, -4, "more than 6 semitones apart")):
        a = [np.zeros(1, dtype=np.int64), i32(5000), i32(1), i32(1), i32(pitch), np.zeros(1, dtype=np.uint8), None if step is None else i32(step), np.zeros(1, dtype=np.int64)]
        p = [None if v is None else C.c_void_p(v.ctypes.data) for v in a]
        rc = lib.f5hip_wave_prosody_shape(1, C.c_void_p(pcm.data_ptr()), p[0], p[1], None, p[2], p[3], p[4], p[5], p[6], None, C.c_void_p(out.data_ptr()), p[7],
                                          C.c_void_p(lens.data_ptr()), _lib.current_stream_ptr())
        assert rc != 0 and text.encode() in lib.f5hip_last_error(), text
    for pitch, step, n, text in ((0, 7, 1, "formant step of 7"), (3, -4, 1, "formant step of -4"), (3, -3, 2, "formant needs one value per request")):
        with pytest.raises(RuntimeError, match=text):
            torch.ops.f5hip.wave_prosody_shape(pcm, torch.zeros(1, dtype=torch.int64), t32(5000), None, t32(1), t32(1), t32(pitch), torch.zeros(1, dtype=torch.uint8),
                                               torch.full((n,), step, dtype=torch.int32), None)
    torch.cuda.synchronize()
    assert _counter("wave_prosody_launches") == 0 and _counter("wave_formant_launches") == 0 and bool((out == 77).all()) and lens.item() == -5


def test_one_micro_batch_makes_one_prosody_call():
    dev = lambda x: torch.from_numpy(x.astype(np.float32) / 32768.0).to("cuda:0")   # noqa: E731
    reqs = [[dev(vowel(20000, 110))], [dev(content("mixed", 14000))], [dev(vowel(9000, 150))]]
    opts = dict(tempo=[1.25, None, 0.8], pitch=[{"semitones": 4, "formant": -2}, 3, -2], keep_formants=[None, None, True], watermark=99, loudness=-20.0)
    want = infer.finish_requests([[w.cpu().numpy() for w in r] for r in reqs], ["x"] * 3, **opts)
    infer.backend_stats.clear()
    _reset()
    got = infer.finish_requests(reqs, ["x"] * 3, device_backend=True, want="pcm16", **opts)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and infer.backend_stats["prosody_calls"] == 1 and infer.backend_stats["host_requests"] == 0
    assert _counter("wave_prosody_launches") == 2 and _counter("wave_formant_launches") == 3 and _counter("wave_formant_requests") == 2


def test_on_a_callers_stream():
    from test_gpu_streams import _pcm_case, _valid

    def run(pcm, offsets, lens, len_dev):
        pcm2, len2, off2, _ = ops.wave_prosody(pcm, offsets, lens, len_dev, [(1, 1), (5, 4), (1, 1)], [3, 0, -2], [False, False, True], [-3, 4, 0])
        return [len2] + _valid(pcm2, off2, len2)
    _pcm_case("wave_prosody formant", run)
