"""The per-voice denoiser of uploaded reference clips on the device (csrc/ref_denoise.h, f5hip_ref_denoise: a ragged STFT, an exact per-bin
order statistic, the gain stage with the inverse FFT and the overlap-add, four launches, in place) against its definition in float64
(tests/denoise_ref.py, the restatement `audio_prep.denoise_reference` is tested against), then batch invariance, the two bindings, the
refusals and the way through `F5HipModel.prepare_voices` and `TTSManager.synthesize_clip(..., denoise=True)`.

The tolerance of a clip is computed, not fixed: 16 times the maximum error of the float32 run of tests/denoise_ref.py on the same clip
(room for ten radix-2 stages with table twiddles against pocketfft's fewer, plus the gain quotient), and never above the project's 1e-4
waveform bound."""
import ctypes as C
import io
import threading
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import denoise_ref as R  # noqa: E402
from tts_indic_server_f5_amd import _lib, audio_prep, infer, ops, serve, synth  # noqa: E402

DEV = "cuda:0"
GAP = 37
SENTINEL = 7.5


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _clips():
    """name -> float32 clip: the nine lengths, an all-zero clip, a DC clip and a clip at peak 1e-4."""
    clips = {f"n{n}": R.clip(n) for n in R.LENGTHS}
    clips["zeros5000"] = np.zeros(5000, dtype=np.float32)
    clips["dc3000"] = np.full(3000, 0.25, dtype=np.float32)
    quiet = R.noisy_speech(20000, 77)[1]
    clips["peak1e-4"] = (quiet * (1e-4 / np.abs(quiet).max())).astype(np.float32)
    return clips


def bound_of(x):
    """(float64 definition of x, the clip's tolerance): 16 times the float32 run's maximum error, at most 1e-4."""
    want = R.denoise(x.astype(np.float64), np.float64)
    err32 = float(np.abs(R.denoise(x, np.float32).astype(np.float64) - want).max())
    return want, err32, min(16.0 * err32, 1e-4)


class Batch:
    """One ragged call over all clips, packed with gaps of sentinel samples between them and a clip left out of the table behind them."""

    def __init__(self):
        self.clips = _clips()
        self.names = list(self.clips)
        self.left_out = R.clip(1000, 5)
        at, self.offsets = GAP, []
        for x in self.clips.values():
            self.offsets.append(at)
            at += len(x) + GAP
        self.left_at = at
        total = at + len(self.left_out) + GAP
        host = np.full(total, SENTINEL, dtype=np.float32)
        for off, x in zip(self.offsets, self.clips.values()):
            host[off:off + len(x)] = x
        host[self.left_at:self.left_at + len(self.left_out)] = self.left_out
        self.before = host
        wave_dev = torch.from_numpy(host).to(DEV)
        _reset()
        ops.ref_denoise(wave_dev, self.offsets, [len(x) for x in self.clips.values()])
        self.launches, self.counted = _counter("ref_denoise_launches"), _counter("ref_denoise_clips")
        self.after = wave_dev.cpu().numpy()
        self.refs = {name: bound_of(x) for name, x in self.clips.items()}     # computed once, shared, never written

    def got(self, name):
        off = self.offsets[self.names.index(name)]
        return self.after[off:off + len(self.clips[name])]


@pytest.fixture(scope="module")
def batch():
    return Batch()


NAMES = [f"n{n}" for n in R.LENGTHS] + ["zeros5000", "dc3000", "peak1e-4"]


def test_ragged_batch_is_four_launches(batch):
    assert batch.names == NAMES
    assert batch.launches == 4 and batch.counted == len(NAMES)
    assert np.isfinite(batch.after).all()
    assert not batch.got("zeros5000").any()                                     # a silent clip stays silent


@pytest.mark.parametrize("name", NAMES)
def test_clip_meets_its_computed_tolerance(batch, name):
    want, err32, bound = batch.refs[name]
    got = batch.got(name).astype(np.float64)
    err = float(np.abs(got - want).max())
    print(f"[ref_denoise] {name}: n={len(want)} F={R.n_frames(len(want))} device max |err| {err:.3e}; float32 run {err32:.3e}; bound {bound:.3e}")
    assert bound <= 1e-4
    assert err <= bound


def test_every_clip_equals_its_single_clip_call(batch):
    for name in NAMES:
        x = batch.clips[name]
        solo = torch.from_numpy(x).to(DEV)
        ops.ref_denoise(solo, [0], [len(x)])
        assert np.array_equal(solo.cpu().numpy().view(np.uint32), batch.got(name).view(np.uint32)), name


def test_gaps_and_clips_left_out_keep_their_bits(batch):
    touched = np.zeros(len(batch.before), dtype=bool)
    for off, name in zip(batch.offsets, NAMES):
        touched[off:off + len(batch.clips[name])] = True
    assert np.array_equal(batch.after[~touched].view(np.uint32), batch.before[~touched].view(np.uint32))
    assert np.array_equal(batch.after[batch.left_at:batch.left_at + 1000], batch.left_out)
    assert (~touched).sum() == GAP * (len(NAMES) + 2) + 1000


def test_ctypes_and_operator_paths_return_the_same_bits(batch):
    order = [5, 0, 8, 3]                                                         # the table need not be in address order
    off = np.array([batch.offsets[i] for i in order], dtype=np.int64)
    ln = np.array([len(batch.clips[NAMES[i]]) for i in order], dtype=np.int32)
    a, b, c = (torch.from_numpy(batch.before).to(DEV) for _ in range(3))
    _lib.check(_lib.lib().f5hip_ref_denoise(len(ln), C.c_void_p(off.ctypes.data), C.c_void_p(ln.ctypes.data), C.c_void_p(a.data_ptr()),
                                            _lib.current_stream_ptr()), "f5hip_ref_denoise")
    assert torch.ops.f5hip.ref_denoise(b, torch.from_numpy(off), torch.from_numpy(ln)) is None
    assert ops.ref_denoise(c, off, ln) is c
    assert torch.equal(a, b) and torch.equal(a, c)
    got = a.cpu().numpy()
    for i in order:
        o, n = batch.offsets[i], len(batch.clips[NAMES[i]])
        assert np.array_equal(got[o:o + n].view(np.uint32), batch.got(NAMES[i]).view(np.uint32))
    left = np.ones(len(got), dtype=bool)
    for i in order:
        left[batch.offsets[i]:batch.offsets[i] + len(batch.clips[NAMES[i]])] = False
    assert np.array_equal(got[left].view(np.uint32), batch.before[left].view(np.uint32))


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    wave_dev = torch.full((4096,), 0.5, device=DEV)
    limit = audio_prep.DENOISE_MAX_SAMPLES

    def call(n, off, ln, wave_ptr=wave_dev.data_ptr(), null_tables=False):
        a, b = np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int32)
        return lib.f5hip_ref_denoise(n, None if null_tables else C.c_void_p(a.ctypes.data), None if null_tables else C.c_void_p(b.ctypes.data),
                                     C.c_void_p(wave_ptr) if wave_ptr else None, _lib.current_stream_ptr())

    _reset()
    assert call(0, [0], [16]) != 0                                               # fewer than one clip
    assert call(2, [0, 100], [16, 0]) != 0                                       # a length below 1
    assert call(1, [0], [limit + 1]) != 0                                        # a length above the limit
    assert call(2, [0, -4], [16, 2]) != 0                                        # a negative offset
    assert call(2, [0, 15], [16, 4]) != 0                                        # overlapping ranges
    assert call(3, [64, 0, 64], [8, 8, 1]) != 0
    assert call(1, [0], [16], wave_ptr=0) != 0                                   # null pointers
    assert call(1, [0], [16], null_tables=True) != 0
    many = (2 ** 31 - 1) // audio_prep.denoise_frames(limit) + 1                 # more than 2^31 - 1 frame rows
    assert call(many, np.arange(many, dtype=np.int64) * limit, np.full(many, limit, dtype=np.int32)) != 0
    assert lib.f5hip_last_error()
    i64, i32 = (lambda v: torch.tensor(v, dtype=torch.int64)), (lambda v: torch.tensor(v, dtype=torch.int32))
    for off, ln in (([], []), ([0, 100], [16, 0]), ([0], [limit + 1]), ([0, -4], [16, 2]), ([0, 15], [16, 4]), ([4090], [16]), ([0, 1], [16])):
        with pytest.raises(_lib.F5HipError):
            ops.ref_denoise(wave_dev, off, ln)
        with pytest.raises(RuntimeError):
            torch.ops.f5hip.ref_denoise(wave_dev, i64(off), i32(ln))
    for bad in (wave_dev.cpu(), wave_dev.double(), wave_dev.view(64, 64), wave_dev[::2]):
        with pytest.raises(_lib.F5HipError):
            ops.ref_denoise(bad, [0], [16])
    assert _counter("ref_denoise_launches") == 0 and _counter("ref_denoise_clips") == 0
    torch.cuda.synchronize()
    assert bool((wave_dev == 0.5).all())                                         # and nothing was written
    assert call(1, [8], [16]) == 0 and _counter("ref_denoise_launches") == 4 and _counter("ref_denoise_clips") == 1


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)
VOCAB = {chr(32 + i): i for i in range(96)}
REF_TEXT, TEXT = "Some call me nature", "I have been a silent spectator."


@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def _upload(seconds, seed, sr=24000):
    x = R.noisy_speech(int(seconds * R.RATE), seed)[1]
    if sr != R.RATE:
        n = int(seconds * sr)
        x = np.interp(np.arange(n) * (R.RATE / sr), np.arange(len(x)), x)
    return torch.from_numpy(x.astype(np.float32))[None], sr


def test_prepare_voices_denoises_the_flagged_voice_in_place(hip_objects):
    model, _ = hip_objects
    a, b = _upload(2.0, 31, 16000), _upload(1.5, 32, 16000)
    today = model.prepare_voices([infer.PreparedVoice.deferred(a), infer.PreparedVoice.deferred(b)])      # no flag: today's result
    _reset()
    model.prepare_voices([infer.PreparedVoice.deferred(b)])
    assert _counter("ref_denoise_launches") == 0                                 # a batch with no flagged voice makes no denoise call
    flagged, plain = infer.PreparedVoice.deferred(a, denoise=True), infer.PreparedVoice.deferred(b)
    model.prepare_voices([flagged, plain])
    assert _counter("ref_denoise_launches") == 4 and _counter("ref_denoise_clips") == 1
    assert torch.equal(plain.audio, today[1].audio) and torch.equal(plain.mel, today[1].mel) and torch.equal(plain.rms, today[1].rms)
    assert torch.equal(flagged.rms, today[0].rms) and flagged.ref_frames == today[0].ref_frames and flagged.audio.shape == today[0].audio.shape
    x = today[0].audio[0].cpu().numpy()
    want, err32, bound = bound_of(x)
    err = float(np.abs(flagged.audio[0].cpu().numpy().astype(np.float64) - want).max())
    print(f"[ref_denoise] prepare_voices: n={len(x)} device max |err| {err:.3e}; float32 run {err32:.3e}; bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(flagged.mel, model.cond_mel(flagged.audio)) and not torch.equal(flagged.mel, today[0].mel)


def _wav_bytes(clip):
    x, sr = clip
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(infer.quantise_pcm16(x[0].numpy()).tobytes())
    return buf.getvalue()


def test_manager_denoises_a_micro_batch_of_two_uploads_in_one_call(hip_objects, attn_shape_invariant):
    mgr = serve.TTSManager(nfe_step=4, device_frontend=True, micro_batch=dict(max_requests=2, max_wait_ms=20000)).load(*hip_objects)
    try:
        raws = [_wav_bytes(_upload(1.6, 41)), _wav_bytes(_upload(1.3, 42))]

        def both(**kw):
            out = [None, None]
            threads = [threading.Thread(target=lambda i=i: out.__setitem__(i, mgr.synthesize_clip(TEXT, raws[i], REF_TEXT, seed=3 + i, **kw))) for i in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            return out

        _reset()
        first = both(denoise=True)
        assert mgr.batcher.batch_sizes == [2]
        assert _counter("ref_denoise_launches") == 4 and _counter("ref_denoise_clips") == 2       # one call for the two flagged uploads
        again = both(denoise=True)
        assert _counter("ref_denoise_launches") == 4                                              # the cached voices are not denoised again
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        plain = both()
        assert _counter("ref_denoise_launches") == 4 and len(mgr._clip_cache) == 4
        assert all(x.shape == y.shape and not np.array_equal(x, y) for x, y in zip(first, plain))
    finally:
        mgr.close()
