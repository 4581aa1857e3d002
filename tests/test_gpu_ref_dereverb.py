"""The per-voice dereverberator of uploaded reference clips on the device (csrc/ref_dereverb.h, f5hip_ref_dereverb: the denoiser's ragged STFT,
one WPE kernel -- fp32 MFMA Gram accumulation over frame chunks, a 16 x 16 complex Cholesky solve and the filter, three iterations -- the
inverse FFT and the overlap-add, four launches, in place) against its definition in float64 (tests/dereverb_ref.py), then batch invariance,
the two bindings, the refusals and the way through `F5HipModel.prepare_voices`.

The tolerance of a clip is the denoiser's rule: 16 times the maximum error of the float32 run of tests/dereverb_ref.py on the same clip (room
for radix-2 table twiddles, the MFMA's summation order and Cholesky against LAPACK's LU), and never above the project's 1e-4 waveform bound.
Every clip's peak is at most 0.5, and tests/test_dereverb_host.py checks that the float32 run stays under 1e-4 / 16 on each of them, so the cap
hides nothing.  Measured, float32 run / device: 0 / 0 (one sample, zeros), 3.0e-8 / 3.0e-8 and 4.5e-8 (F = 4, 5), 4.1e-6 / 5.2e-6 and 4.5e-6
(F = 19, 20: white noise, as many taps as frames), 7.4e-7 / 6.8e-7 (F = 129), 9.8e-7 / 6.2e-7 (1.5 s), 2.7e-6 / 2.9e-6 (DC)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dereverb_ref as R  # noqa: E402
from tts_indic_server_f5_amd import _lib, audio_prep, infer, ops, synth  # noqa: E402

DEV = "cuda:0"
GAP = 37
SENTINEL = 7.5


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def bound_of(x):
    """(float64 definition of x, the float32 run's maximum error, the clip's tolerance)."""
    want = R.dereverb(x.astype(np.float64), np.float64)
    err32 = float(np.abs(R.dereverb(x, np.float32).astype(np.float64) - want).max())
    return want, err32, min(16.0 * err32, 1e-4)


class Batch:
    """One ragged call over all clips, packed with gaps of sentinel samples between them and a clip left out of the table behind them."""

    def __init__(self):
        self.clips = R.device_clips(ops.ref_dereverb_chunk())
        self.names = list(self.clips)
        self.lengths = [len(x) for x in self.clips.values()]
        self.left_out = self.clips["short_one_tap"].copy()
        at, self.offsets = GAP, []
        for n in self.lengths:
            self.offsets.append(at)
            at += n + GAP
        self.left_at = at
        host = np.full(at + len(self.left_out) + GAP, SENTINEL, dtype=np.float32)
        for off, x in zip(self.offsets, self.clips.values()):
            host[off:off + len(x)] = x
        host[self.left_at:self.left_at + len(self.left_out)] = self.left_out
        self.before = host
        wave_dev = torch.from_numpy(host).to(DEV)
        _reset()
        ops.ref_dereverb(wave_dev, self.offsets, self.lengths)
        self.launches, self.counted = _counter("ref_dereverb_launches"), _counter("ref_dereverb_clips")
        self.after = wave_dev.cpu().numpy()
        self.refs = {name: bound_of(x) for name, x in self.clips.items()}     # computed once, shared, never written

    def got(self, name, wave=None):
        i = self.names.index(name)
        return (self.after if wave is None else wave)[self.offsets[i]:self.offsets[i] + self.lengths[i]]


@pytest.fixture(scope="module")
def batch():
    return Batch()


NAMES = ["one_sample", "no_tap", "short_one_tap", "line_short_by_one", "line_full", "chunk_plus_one", "seconds_1p5", "zeros", "dc"]


def test_ragged_batch_is_one_call_of_the_declared_launches(batch):
    chunk = ops.ref_dereverb_chunk()
    frames = [R.n_frames(n) for n in batch.lengths]
    assert batch.names == NAMES and frames[:7] == [4, R.DELAY, R.DELAY + 1, R.DELAY + R.TAPS - 1, R.DELAY + R.TAPS, chunk + 1, 144]
    assert batch.launches == ops.ref_dereverb_launches() == 4 and batch.counted == len(NAMES)
    assert np.isfinite(batch.after).all()
    assert not batch.got("zeros").any()                                          # a silent clip stays silent


@pytest.mark.parametrize("name", NAMES)
def test_clip_meets_its_computed_tolerance(batch, name):
    want, err32, bound = batch.refs[name]
    err = float(np.abs(batch.got(name).astype(np.float64) - want).max())
    print(f"[ref_dereverb] {name}: n={len(want)} F={R.n_frames(len(want))} device max |err| {err:.3e}; float32 run {err32:.3e}; bound {bound:.3e}")
    assert np.abs(batch.clips[name]).max() <= 0.5 and err32 <= 1e-4 / 16
    assert err <= bound


def test_every_clip_equals_its_single_clip_call_and_any_table_order(batch):
    for name in NAMES:
        solo = torch.from_numpy(batch.clips[name]).to(DEV)
        ops.ref_dereverb(solo, [0], [len(solo)])
        assert np.array_equal(solo.cpu().numpy().view(np.uint32), batch.got(name).view(np.uint32)), name
    order = [6, 0, 8, 3, 5, 1, 7, 2, 4]
    again = torch.from_numpy(batch.before).to(DEV)
    ops.ref_dereverb(again, [batch.offsets[i] for i in order], [batch.lengths[i] for i in order])
    assert np.array_equal(again.cpu().numpy().view(np.uint32), batch.after.view(np.uint32))


def test_gaps_and_clips_left_out_keep_their_bits(batch):
    touched = np.zeros(len(batch.before), dtype=bool)
    for off, n in zip(batch.offsets, batch.lengths):
        touched[off:off + n] = True
    assert np.array_equal(batch.after[~touched].view(np.uint32), batch.before[~touched].view(np.uint32))
    assert (~touched).sum() == GAP * (len(NAMES) + 2) + len(batch.left_out)


def test_ctypes_and_operator_paths_return_the_same_bits(batch):
    order = [5, 0, 8, 3]                                                         # the table need not be in address order
    off = np.array([batch.offsets[i] for i in order], dtype=np.int64)
    ln = np.array([batch.lengths[i] for i in order], dtype=np.int32)
    a, b, c = (torch.from_numpy(batch.before).to(DEV) for _ in range(3))
    _lib.check(_lib.lib().f5hip_ref_dereverb(len(ln), C.c_void_p(off.ctypes.data), C.c_void_p(ln.ctypes.data), C.c_void_p(a.data_ptr()),
                                             _lib.current_stream_ptr()), "f5hip_ref_dereverb")
    assert torch.ops.f5hip.ref_dereverb(b, torch.from_numpy(off), torch.from_numpy(ln)) is None
    assert ops.ref_dereverb(c, off, ln) is c
    assert torch.equal(a, b) and torch.equal(a, c)
    got = a.cpu().numpy()
    left = np.ones(len(got), dtype=bool)
    for i in order:
        assert np.array_equal(batch.got(NAMES[i], got).view(np.uint32), batch.got(NAMES[i]).view(np.uint32))
        left[batch.offsets[i]:batch.offsets[i] + batch.lengths[i]] = False
    assert np.array_equal(got[left].view(np.uint32), batch.before[left].view(np.uint32))


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    wave_dev = torch.full((4096,), 0.5, device=DEV)
    limit = audio_prep.DEREVERB_MAX_SAMPLES

    def call(n, off, ln, wave_ptr=wave_dev.data_ptr(), null_tables=False):
        a, b = np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int32)
        return lib.f5hip_ref_dereverb(n, None if null_tables else C.c_void_p(a.ctypes.data), None if null_tables else C.c_void_p(b.ctypes.data),
                                      C.c_void_p(wave_ptr) if wave_ptr else None, _lib.current_stream_ptr())

    _reset()
    many = (2 ** 31 - 1) // audio_prep.denoise_frames(limit) + 1                 # more than 2^31 - 1 frame rows
    refused = [(0, [0], [16]), (2, [0, 100], [16, 0]), (1, [0], [limit + 1]), (2, [0, -4], [16, 2]), (2, [0, 15], [16, 4]), (3, [64, 0, 64], [8, 8, 1]),
               (many, np.arange(many, dtype=np.int64) * limit, np.full(many, limit, dtype=np.int32))]
    assert all(call(*r) != 0 for r in refused)
    assert call(1, [0], [16], wave_ptr=0) != 0 and call(1, [0], [16], null_tables=True) != 0      # null pointers
    assert lib.f5hip_last_error()
    i64, i32 = (lambda v: torch.tensor(v, dtype=torch.int64)), (lambda v: torch.tensor(v, dtype=torch.int32))
    for off, ln in (([], []), ([0, 100], [16, 0]), ([0], [limit + 1]), ([0, -4], [16, 2]), ([0, 15], [16, 4]), ([4090], [16]), ([0, 1], [16])):
        with pytest.raises(_lib.F5HipError):
            ops.ref_dereverb(wave_dev, off, ln)
        with pytest.raises(RuntimeError):
            torch.ops.f5hip.ref_dereverb(wave_dev, i64(off), i32(ln))
    for bad in (wave_dev.cpu(), wave_dev.double(), wave_dev.view(64, 64), wave_dev[::2]):
        with pytest.raises(_lib.F5HipError):
            ops.ref_dereverb(bad, [0], [16])
    assert _counter("ref_dereverb_launches") == 0 and _counter("ref_dereverb_clips") == 0
    torch.cuda.synchronize()
    assert bool((wave_dev == 0.5).all())                                         # and nothing was written
    assert call(1, [8], [16]) == 0 and _counter("ref_dereverb_launches") == 4 and _counter("ref_dereverb_clips") == 1


ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)


def test_prepare_voices_dereverberates_the_flagged_voice_in_place():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    model = F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map={chr(32 + i): i for i in range(96)})
    a, b = ((torch.from_numpy(R.host(s, 0.3, seed)[0].astype(np.float32))[None], 24000) for s, seed in ((1.2, 31), (1.0, 32)))
    today = model.prepare_voices([infer.PreparedVoice.deferred(a), infer.PreparedVoice.deferred(b)])      # no flag: today's result
    _reset()
    flagged, plain = infer.PreparedVoice.deferred(a, dereverb=True), infer.PreparedVoice.deferred(b)
    model.prepare_voices([flagged, plain])
    assert _counter("ref_dereverb_launches") == 4 and _counter("ref_dereverb_clips") == 1 and _counter("ref_denoise_launches") == 0
    assert torch.equal(plain.audio, today[1].audio) and torch.equal(plain.mel, today[1].mel) and torch.equal(plain.rms, today[1].rms)
    assert torch.equal(flagged.rms, today[0].rms) and flagged.audio.shape == today[0].audio.shape
    x = today[0].audio[0].cpu().numpy()
    want, err32, bound = bound_of(x)
    err = float(np.abs(flagged.audio[0].cpu().numpy().astype(np.float64) - want).max())
    print(f"[ref_dereverb] prepare_voices: n={len(x)} peak {np.abs(x).max():.2f} device max |err| {err:.3e}; float32 run {err32:.3e}; bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(flagged.mel, model.cond_mel(flagged.audio)) and not torch.equal(flagged.mel, today[0].mel)
