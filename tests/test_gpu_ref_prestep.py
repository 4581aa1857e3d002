"""The reference-clip pre-step on the device (csrc/ref_prestep.h, f5hip_ref_prestep: clip at a pause, strip the silent edges, 50 ms tail for
a ragged batch of int16 clips in three launches) against its definition, `audio_prep.preprocess_ref_segment`, bit for bit on the case
matrix of tests/ref_prestep_cases.py; then the hand-off to `ops.ref_frontend`, the ctypes and operator paths, the refusals, and
`TTSManager(device_prestep=True)` end to end on a tiny model.  Everything is an equality: there is no tolerance in this file."""
import ctypes as C
import functools
import io
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_prestep_cases as RC  # noqa: E402
from tts_indic_server_f5_amd import _lib, infer, ops, serve, synth  # noqa: E402

DEV = "cuda:0"
NAMES = list(RC.cases())
RATES = sorted({rate for _, rate, _ in RC.cases().values()})


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _call(names):
    """ops.ref_prestep on the named cases in one call -> [(planes [ch, n] numpy, length, flag)]"""
    items = [RC.cases()[n] for n in names]
    rate = items[0][1]
    assert all(r == rate for _, r, _ in items)
    frames = np.concatenate([x.reshape(-1) for x, _, _ in items])
    channels = [x.shape[1] for x, _, _ in items]
    packed, lengths, flags = ops.ref_prestep(frames, [x.shape[0] for x, _, _ in items], channels, rate, [c for _, _, c in items], device=DEV)
    assert packed.is_cuda and packed.dtype == torch.float32 and packed.numel() == sum(n * c for n, c in zip(lengths, channels))
    return [(p.cpu().numpy(), n, f) for p, n, f in zip(ops.ref_prestep_planes(packed, lengths, channels), lengths, flags)]


@functools.lru_cache(maxsize=None)
def _solo(name):
    return _call([name])[0]


def _want(name):
    frames = RC.expected(name)
    return np.ascontiguousarray((frames.astype(np.float32) / 32768.0).T), frames.shape[0], bool(frames.any())


@pytest.mark.parametrize("name", NAMES)
def test_every_case_alone_equals_the_host_function(name):
    planes, length, flag = _solo(name)
    want, n, nonzero = _want(name)
    print(f"[ref_prestep] {name}: {RC.cases()[name][0].shape[0]} frames in, {length} out (host {n}), non-zero {flag}")
    assert (length, flag) == (n, nonzero)
    assert planes.shape == want.shape and torch.equal(torch.from_numpy(planes), torch.from_numpy(want))


@pytest.mark.parametrize("rate", RATES)
def test_all_cases_of_one_rate_in_one_call(rate):
    names = [n for n in NAMES if RC.cases()[n][1] == rate]
    _reset()
    got = _call(names)
    assert _counter("ref_prestep_launches") == 3 and _counter("ref_prestep_clips") == len(names)      # three launches whatever the batch
    for name, (planes, length, flag) in zip(names, got):
        solo = _solo(name)
        assert (length, flag) == solo[1:], name
        assert np.array_equal(planes.view(np.uint32), solo[0].view(np.uint32)), name


def test_the_front_end_reads_the_output_in_place():
    names = ["edges_two_ranges", "ms_999", "thresh_edges_260", "lead_37"]
    items = [RC.cases()[n] for n in names]
    frames = np.concatenate([x.reshape(-1) for x, _, _ in items])
    channels = [x.shape[1] for x, _, _ in items]
    packed, lengths, _ = ops.ref_prestep(frames, [x.shape[0] for x, _, _ in items], channels, 11025, [c for _, _, c in items], device=DEV)
    taps = infer.resample_taps(11025, 24000)[3].to(DEV)
    out, rms, n_out = ops.ref_frontend(packed, lengths, channels, 11025, 24000, taps, 0.1)
    host = torch.from_numpy(np.concatenate([_want(n)[0].reshape(-1) for n in names])).to(DEV)           # host pre-step, then the upload
    out_h, rms_h, n_out_h = ops.ref_frontend(host, [_want(n)[1] for n in names], channels, 11025, 24000, taps, 0.1)
    assert n_out == n_out_h and torch.equal(out, out_h) and torch.equal(rms, rms_h)


def test_ctypes_and_operator_paths_return_the_same_bits():
    names = ["thresh_pass1_103", "ms_999", "zero_frames", "edges_two_ranges"]
    items = [RC.cases()[n] for n in names]
    ni = np.array([x.shape[0] for x, _, _ in items], dtype=np.int32)
    ch = np.array([x.shape[1] for x, _, _ in items], dtype=np.int32)
    cs = np.array([c for _, _, c in items], dtype=np.uint8)
    frames = torch.from_numpy(np.concatenate([x.reshape(-1) for x, _, _ in items])).to(DEV)
    lib = _lib.lib()
    bound = lib.f5hip_ref_prestep_bound(len(ni), C.c_void_p(ni.ctypes.data), C.c_void_p(ch.ctypes.data), 11025)
    assert bound == int(((ni.astype(np.int64) + 551) * ch).sum())
    out = torch.full((bound,), float("nan"), device=DEV)
    info = torch.full((len(ni), 2), -7, device=DEV, dtype=torch.int32)
    _lib.check(lib.f5hip_ref_prestep(len(ni), C.c_void_p(ni.ctypes.data), C.c_void_p(ch.ctypes.data), C.c_void_p(cs.ctypes.data),
                                     C.c_void_p(frames.data_ptr()), frames.numel(), 11025, C.c_void_p(out.data_ptr()), C.c_void_p(info.data_ptr()),
                                     _lib.current_stream_ptr()), "f5hip_ref_prestep")
    out_op, info_op = torch.ops.f5hip.ref_prestep(frames, torch.from_numpy(ni), torch.from_numpy(ch), torch.from_numpy(cs), 11025)
    assert torch.equal(info, info_op)
    used = int((info[:, 0].cpu().numpy().astype(np.int64) * ch).sum())
    assert torch.equal(out[:used], out_op[:used])
    at = 0
    for name, c, (n, flag) in zip(names, ch, info.cpu().numpy()):
        want, length, nonzero = _want(name)
        assert (int(n), bool(flag)) == (length, nonzero), name
        assert torch.equal(out[at:at + n * c].cpu().view(int(c), int(n)), torch.from_numpy(want)), name
        at += int(n) * int(c)


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    frames = torch.zeros(64, device=DEV, dtype=torch.int16)
    out, info = torch.zeros(8192, device=DEV), torch.zeros(8, device=DEV, dtype=torch.int32)

    def call(n, n_in, ch, rate, n_samples=64):
        a, b, c = np.asarray(n_in, dtype=np.int32), np.asarray(ch, dtype=np.int32), np.ones(len(n_in), dtype=np.uint8)
        return lib.f5hip_ref_prestep(n, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(frames.data_ptr()),
                                     n_samples, rate, C.c_void_p(out.data_ptr()), C.c_void_p(info.data_ptr()), _lib.current_stream_ptr())

    _reset()
    assert call(0, [64], [1], 16000) != 0                                  # fewer than one clip
    assert call(1, [64], [1], 11024) != 0                                  # a rate below 11 025
    assert call(2, [32, 32], [1, 0], 16000) != 0                           # a channel count below 1
    assert call(2, [32, 31], [1, 1], 16000) != 0                           # counts that do not add up to the buffer's size
    assert call(1, [16], [2], 16000) != 0
    assert call(2, [2 ** 31 - 1, 2 ** 31 - 1], [1, 1], 16000, 2 ** 32 - 2) != 0    # more than 2^31 - 1 samples
    assert call(1, [-1], [1], 16000, -1) != 0
    assert lib.f5hip_last_error()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    for n_in, ch, rate in (([], [], 16000), ([64], [1], 11024), ([32, 32], [1, 0], 16000), ([32, 31], [1, 1], 16000)):
        with pytest.raises(_lib.F5HipError):
            ops.ref_prestep(frames, n_in, ch, rate)
        with pytest.raises(RuntimeError):
            torch.ops.f5hip.ref_prestep(frames, i32(n_in), i32(ch), torch.ones(len(n_in), dtype=torch.uint8), rate)
    assert _counter("ref_prestep_launches") == 0
    assert call(1, [32], [2], 16000) == 0 and _counter("ref_prestep_launches") == 3
    torch.cuda.synchronize()
    assert info[:2].tolist() == [800, 0]                                   # zeros in: the 50 ms tail alone, flagged all-zero


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)
VOCAB = {chr(32 + i): i for i in range(96)}
REF_TEXT, TEXT = "Some call me nature", "I have been a silent spectator. Always remember, I endure."


def _wav_bytes(frames, sr):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(frames.shape[1]); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(np.ascontiguousarray(frames, dtype="<i2").tobytes())
    return buf.getvalue()


@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


@pytest.mark.parametrize("name", ["pass1_stop", "short_44100_stereo"])
def test_manager_returns_the_host_path_bytes(hip_objects, name):
    x, rate, clip = RC.cases()[name]
    raw = _wav_bytes(x, rate)
    waves = []
    for device_prestep in (True, False):
        mgr = serve.TTSManager(nfe_step=8, device_frontend=True, device_prestep=device_prestep).load(*hip_objects)
        _reset()
        waves.append(mgr.synthesize_clip(TEXT, raw, REF_TEXT, clip_short=clip, seed=3))
        assert _counter("ref_prestep_launches") == (3 if device_prestep else 0)      # the device pre-step ran, resp. did not
        voice = mgr._clip_voice(raw, REF_TEXT, clip)[0]
        assert voice.pending is None and voice.audio.is_cuda
    assert waves[0].shape == waves[1].shape and np.array_equal(waves[0], waves[1])


def test_manager_refuses_the_all_zero_clip_with_the_host_message(hip_objects):
    x, rate, clip = RC.cases()["zeros_2s"]
    messages = []
    for device_prestep in (True, False):
        mgr = serve.TTSManager(nfe_step=8, device_frontend=True, device_prestep=device_prestep).load(*hip_objects)
        with pytest.raises(ValueError) as e:
            mgr.synthesize_clip(TEXT, _wav_bytes(x, rate), REF_TEXT)
        messages.append(str(e.value))
    assert messages[0] == messages[1] == "Invalid audio: the clip is empty or silent."


def test_a_script_prepares_its_new_uploads_in_one_call_per_rate(hip_objects, monkeypatch):
    calls = []
    real = ops.ref_prestep

    def counted(frames, n_in, channels, rate, *a, **k):
        calls.append((int(rate), len(n_in)))
        return real(frames, n_in, channels, rate, *a, **k)

    monkeypatch.setattr(ops, "ref_prestep", counted)
    tone = lambda ms, rate, hz, ch=1: _wav_bytes(RC.cat(RC.zeros(60, rate, ch), RC.tone(ms, rate, hz=hz, ch=ch), RC.zeros(120, rate, ch)), rate)
    voices = {"main": dict(ref_audio=tone(1500, 16000, 200.0), ref_text=REF_TEXT),
              "town": dict(ref_audio=tone(1400, 22050, 260.0, 2), ref_text="A town crier"),
              "hill": dict(ref_audio=tone(1600, 16000, 320.0), ref_text="Up on the hill", clip_short=False)}
    script = "I endure. [town] Hear ye. [hill] Always remember. [main] Again."
    got = []
    for device_prestep in (True, False):
        mgr = serve.TTSManager(nfe_step=8, device_frontend=True, device_prestep=device_prestep).load(*hip_objects)
        got.append(mgr.synthesize_script(script, voices, seed=9))
        if device_prestep:
            assert sorted(calls) == [(16000, 2), (22050, 1)]               # three new voices at two rates: two calls
            mgr.synthesize_script(script, voices, seed=9)
            assert len(calls) == 2                                         # all three come from the cache now
    assert len(calls) == 2
    assert got[0].shape == got[1].shape and np.array_equal(got[0], got[1])
