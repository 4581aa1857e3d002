"""The reference-clip report on the device (csrc/ref_assess.h, f5hip_ref_assess: an integer peak and run count on the raw upload, the
denoiser's STFT and order statistic on the prepared wave, frame sums and one block per clip: six launches) against its definition
(audio_prep.assess_reference; tests/assess_ref.py in float64 is the reference), then batch invariance, the launch count, the two bindings, the
refusals and the way through `F5HipModel.prepare_voices` and `TTSManager(reference_limits=...)`.

Counts and the peak must equal the host's exactly.  The tolerance of a float measure is computed per clip, not fixed: 16 times the error of
the float32 run of tests/assess_ref.py against its float64 run -- the room tests/test_gpu_ref_denoise.py gives the same FFT.  `k*` and the
speech frames are threshold decisions: the test finds, in float64, the bins and frames within a relative 1e-3 of their threshold and excludes
only those; the inputs leave no bin near the bandwidth threshold and at most 1 % of a clip's frames near the speech threshold (asserted).

Measured on an MI355X (profiles/ref_assess_parity.txt): noise_db errors of 2.3e-7 .. 5.0e-7 dB against bounds of 4.0e-7 .. 1.6e-4, snr_db 5e-9 .. 9e-7
dB against 3.1e-5 .. 6.6e-4; the tightest is the 255-sample clip, whose float32 run happens to be 2.5e-8 dB off (N: 3.2e-5 against 3.9e-5)."""
import ctypes as C
import io
import math
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import assess_ref as A  # noqa: E402
import denoise_ref as R  # noqa: E402
from tts_indic_server_f5_amd import _lib, audio_prep, infer, ops, serve, synth  # noqa: E402

DEV = "cuda:0"
GAP = 37
SENTINEL = 7.5
BOUNDED = ("N", "S", "noise_db", "snr_db")


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _edge_clip():
    """Stereo, 1000 samples: a run at sample 0, a run of 2, a run that ends at channel 0's last sample, hot samples at channel 1's start
    (not joined to it), a run at channel 1's end; 16-bit tops against -1.0."""
    rng = np.random.default_rng(9)
    x = (0.3 * rng.uniform(-1, 1, (2, 1000))).astype(np.float32)
    top = np.float32(32767 / 32768)
    x[0, 0:4] = [1, top, -1, 1]
    x[0, 100:102] = [1, 1]
    x[0, 500:503] = [-1, -1, top]
    x[0, 997:1000] = [1, 1, 1]
    x[1, 0:2] = [1, 1]
    x[1, 400:407] = [top, top, -1, -1, 1, 1, top]
    x[1, 998:1000] = [1, -1]
    return x                                                                     # clipped = 4 + 3 + 3 + 7 = 17


def _clips():
    """name -> (raw float32 [ch, n], prepared float32 [n])."""
    clips = {}
    for n in R.LENGTHS:
        x = R.clip(n)
        clips[f"n{n}"] = (np.clip(3.0 * x, -1.0, 1.0)[None] if n >= R.SPEECH_FROM else x[None], x)      # the long ones arrive clipped
    clips["zeros5000"] = (np.zeros((1, 5000), dtype=np.float32), np.zeros(5000, dtype=np.float32))
    clips["dc3000"] = (np.full((1, 3000), 0.25, dtype=np.float32), np.full(3000, 0.25, dtype=np.float32))
    edge = _edge_clip()
    clips["stereo_edges"] = (edge, edge.mean(axis=0).astype(np.float32))
    rng = np.random.default_rng(12)
    three = rng.choice(np.array([1.0, -1.0, 32767 / 32768, 0.999, 0.5, -0.2, 0.0], dtype=np.float32), size=(3, 777), p=[.25, .2, .1, .1, .15, .1, .1])
    clips["three_channels"] = (three, three.mean(axis=0).astype(np.float32))
    return clips


NAMES = [f"n{n}" for n in R.LENGTHS] + ["zeros5000", "dc3000", "stereo_edges", "three_channels"]


def _pack(arrays):
    """1-D float32 arrays packed with gaps of sentinel samples -> (host buffer, offsets)."""
    at, offsets = GAP, []
    for a in arrays:
        offsets.append(at)
        at += a.size + GAP
    host = np.full(at, SENTINEL, dtype=np.float32)
    for off, a in zip(offsets, arrays):
        host[off:off + a.size] = a.reshape(-1)
    return host, offsets


def reference_of(raw, prepared):
    """What the device is held to for one clip, computed once: the host's exact values, the float64 restatement, the per-measure bounds
    (16 x the float32 run's error) and the decisions too close to call."""
    peak, clipped = audio_prep.assess_clipping(raw)
    f64, f32 = A.spectrum(prepared.astype(np.float64), np.float64), A.spectrum(prepared, np.float32)
    bounds = {}
    for key in BOUNDED:
        a, b = f64[key], f32[key]
        bounds[key] = 0.0 if a == b else (math.inf if math.isinf(a) or math.isinf(b) else 16.0 * abs(a - b))
    near_bins, near_frames = A.near_thresholds(f64)
    return dict(peak=peak, clipped=clipped, f64=f64, f32=f32, bounds=bounds, near_bins=near_bins, near_frames=near_frames)


class Batch:
    """One ragged call over all clips, both buffers packed with gaps of sentinel samples."""

    def __init__(self):
        self.clips = _clips()
        assert list(self.clips) == NAMES
        self.raw_host, self.raw_off = _pack([raw for raw, _ in self.clips.values()])
        self.wave_host, self.off = _pack([x for _, x in self.clips.values()])
        self.ch = [raw.shape[0] for raw, _ in self.clips.values()]
        self.raw_len = [raw.shape[1] for raw, _ in self.clips.values()]
        self.len = [len(x) for _, x in self.clips.values()]
        self.raw_dev, self.wave_dev = torch.from_numpy(self.raw_host).to(DEV), torch.from_numpy(self.wave_host).to(DEV)
        _reset()
        rows = ops.ref_assess(self.raw_dev, self.raw_off, self.ch, self.raw_len, self.wave_dev, self.off, self.len)
        self.launches, self.counted = _counter("ref_assess_launches"), _counter("ref_assess_clips")
        assert rows.dtype == torch.int64 and tuple(rows.shape) == (len(NAMES), len(audio_prep.ASSESS_ROW)) and rows.is_cuda
        self.rows = rows.cpu().numpy()
        self.refs = {name: reference_of(*clip) for name, clip in self.clips.items()}     # computed once, shared, never written

    def row(self, name):
        row = self.rows[NAMES.index(name)]
        return dict(zip(audio_prep.ASSESS_ROW, row.tolist())), dict(zip(audio_prep.ASSESS_ROW, row.view(np.float64).tolist()))


@pytest.fixture(scope="module")
def batch():
    return Batch()


def test_ragged_batch_is_six_launches(batch):
    assert batch.launches == 6 == _lib.lib().f5hip_ref_assess_launches() and batch.counted == len(NAMES)


def test_buffers_keep_their_bits(batch):
    assert np.array_equal(batch.raw_dev.cpu().numpy().view(np.uint32), batch.raw_host.view(np.uint32))      # gaps, sentinels and clips alike
    assert np.array_equal(batch.wave_dev.cpu().numpy().view(np.uint32), batch.wave_host.view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_counts_and_peak_equal_the_host(batch, name):
    ints, _ = batch.row(name)
    ref = batch.refs[name]
    raw, prepared = batch.clips[name]
    assert ints["peak_bits"] == int(np.array([ref["peak"]], dtype=np.float32).view(np.uint32)[0])
    assert ints["clipped"] == ref["clipped"] == A.clipping(raw)[1]
    report = audio_prep.report_from_row(batch.rows[NAMES.index(name)], 1.0, None, raw.size)
    assert report.peak == float(ref["peak"]) and report.clipped == ref["clipped"] and report.clip_ratio == ref["clipped"] / raw.size
    if name == "stereo_edges":
        assert ints["clipped"] == 17
    if name in ("zeros5000", "dc3000"):
        assert ints["clipped"] == 0
    if name in ("n60000", "three_channels"):
        assert ints["clipped"] > 0


@pytest.mark.parametrize("name", NAMES)
def test_float_measures_meet_their_computed_bounds(batch, name):
    _, got = batch.row(name)
    ref = batch.refs[name]
    failed = []
    for key in BOUNDED:
        want, bound = ref["f64"][key], ref["bounds"][key]
        err = 0.0 if got[key] == want else abs(got[key] - want)
        print(f"[ref_assess] {name}: {key} device {got[key]!r} float64 {want!r} |err| {err:.3e}; float32 run {bound / 16.0:.3e}; bound {bound:.3e}")
        if not err <= bound:
            failed.append(key)
    assert not failed


@pytest.mark.parametrize("name", NAMES)
def test_threshold_decisions_outside_the_excluded_ones(batch, name):
    ints, got = batch.row(name)
    ref = batch.refs[name]
    f64 = ref["f64"]
    print(f"[ref_assess] {name}: F {f64['F']} k* device {ints['k_star']} float64 {f64['k_star']} (bins near the threshold: {ref['near_bins']}); "
          f"speech frames device {ints['speech_frames']} float64 {f64['speech_frames']} (frames near the threshold: {len(ref['near_frames'])})")
    assert ref["near_bins"] == [] and len(ref["near_frames"]) <= 0.01 * f64["F"]          # the inputs' property, checked on the CPU
    assert ints["k_star"] == f64["k_star"] and got["bandwidth_hz"] == f64["bandwidth_hz"]
    assert abs(ints["speech_frames"] - f64["speech_frames"]) <= len(ref["near_frames"])
    assert got["speech_ratio"] == ints["speech_frames"] / f64["F"]


def test_every_row_equals_its_single_clip_call(batch):
    for i, name in enumerate(NAMES):
        raw, x = batch.clips[name]
        solo = ops.ref_assess(torch.from_numpy(raw.reshape(-1).copy()).to(DEV), [0], [raw.shape[0]], [raw.shape[1]], torch.from_numpy(x).to(DEV), [0], [len(x)])
        assert np.array_equal(solo.cpu().numpy()[0], batch.rows[i]), name


def test_ctypes_and_operator_paths_return_the_same_bits(batch):
    order = [12, 5, 0, 8, 11]                                                    # the tables need not be in address order
    pick = lambda v, dt: np.array([v[i] for i in order], dtype=dt)              # noqa: E731
    ro, ch, rl = pick(batch.raw_off, np.int64), pick(batch.ch, np.int32), pick(batch.raw_len, np.int32)
    off, ln = pick(batch.off, np.int64), pick(batch.len, np.int32)
    a = torch.empty(len(order), len(audio_prep.ASSESS_ROW), dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr())      # noqa: E731
    _lib.check(_lib.lib().f5hip_ref_assess(len(order), p(batch.raw_dev), p(ro), p(ch), p(rl), p(batch.wave_dev), p(off), p(ln), p(a), _lib.current_stream_ptr()),
               "f5hip_ref_assess")
    b = torch.ops.f5hip.ref_assess(batch.raw_dev, torch.from_numpy(ro), torch.from_numpy(ch), torch.from_numpy(rl), batch.wave_dev, torch.from_numpy(off),
                                   torch.from_numpy(ln))
    c = ops.ref_assess(batch.raw_dev, ro, ch, rl, batch.wave_dev, off, ln)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert np.array_equal(a.cpu().numpy(), batch.rows[order])


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    raw, wav = torch.full((4096,), 0.5, device=DEV), torch.full((4096,), 0.25, device=DEV)
    rows = torch.full((4, len(audio_prep.ASSESS_ROW)), -7, dtype=torch.int64, device=DEV)
    limit = audio_prep.ASSESS_MAX_SAMPLES

    def call(n, ro, ch, rl, off, ln, raw_ptr=raw.data_ptr(), wave_ptr=wav.data_ptr(), rows_ptr=rows.data_ptr(), null_tables=False):
        t = [np.asarray(ro, dtype=np.int64), np.asarray(ch, dtype=np.int32), np.asarray(rl, dtype=np.int32), np.asarray(off, dtype=np.int64),
             np.asarray(ln, dtype=np.int32)]
        q = [None if null_tables else C.c_void_p(a.ctypes.data) for a in t]
        v = lambda ptr: C.c_void_p(ptr) if ptr else None                         # noqa: E731
        return lib.f5hip_ref_assess(n, v(raw_ptr), q[0], q[1], q[2], v(wave_ptr), q[3], q[4], v(rows_ptr), _lib.current_stream_ptr())

    _reset()
    assert call(0, [0], [1], [16], [0], [16]) != 0                               # fewer than one clip
    assert call(4097, [0], [1], [16], [0], [16]) != 0                            # more than the cap
    assert call(1, [0], [0], [16], [0], [16]) != 0                               # channels outside 1 .. 8
    assert call(1, [0], [9], [16], [0], [16]) != 0
    assert call(2, [0, 100], [1, 1], [16, 0], [0, 100], [16, 16]) != 0           # an empty raw clip
    assert call(2, [0, 100], [1, 1], [16, 16], [0, 100], [16, 0]) != 0           # an empty prepared clip
    assert call(1, [0], [1], [16], [0], [limit + 1]) != 0                        # a prepared length above the limit
    assert call(2, [0, -4], [1, 1], [16, 2], [0, 100], [16, 16]) != 0            # negative offsets
    assert call(2, [0, 100], [1, 1], [16, 2], [0, -1], [16, 16]) != 0
    assert call(2, [0, 30], [2, 1], [16, 4], [0, 100], [16, 16]) != 0            # the second channel of raw clip 0 reaches into clip 1
    assert call(2, [0, 100], [1, 1], [16, 4], [0, 15], [16, 16]) != 0            # overlapping prepared ranges
    assert call(1, [0], [1], [16], [0], [16], raw_ptr=0) != 0                    # null buffers
    assert call(1, [0], [1], [16], [0], [16], wave_ptr=0) != 0
    assert call(1, [0], [1], [16], [0], [16], rows_ptr=0) != 0
    assert call(1, [0], [1], [16], [0], [16], null_tables=True) != 0
    assert lib.f5hip_last_error()
    i64, i32 = (lambda v: torch.tensor(v, dtype=torch.int64)), (lambda v: torch.tensor(v, dtype=torch.int32))
    for ro, ch, rl, off, ln in (([], [], [], [], []), ([0], [9], [16], [0], [16]), ([0], [1], [0], [0], [16]), ([4090], [1], [16], [0], [16]),
                                ([0], [2], [2049], [0], [16]), ([0], [1], [16], [4090], [16]), ([0], [1], [16], [0], [limit + 1]), ([0, 8], [1, 1], [16, 16], [0, 100], [16, 16]),
                                ([0], [1, 1], [16], [0], [16])):
        with pytest.raises(_lib.F5HipError):
            ops.ref_assess(raw, ro, ch, rl, wav, off, ln)
        with pytest.raises(RuntimeError):
            torch.ops.f5hip.ref_assess(raw, i64(ro), i32(ch), i32(rl), wav, i64(off), i32(ln))
    for bad in (raw.cpu(), raw.double(), raw.view(64, 64), raw[::2]):
        with pytest.raises(_lib.F5HipError):
            ops.ref_assess(bad, [0], [1], [16], wav, [0], [16])
        with pytest.raises(_lib.F5HipError):
            ops.ref_assess(raw, [0], [1], [16], bad, [0], [16])
    assert _counter("ref_assess_launches") == 0 and _counter("ref_assess_clips") == 0
    torch.cuda.synchronize()
    assert bool((rows == -7).all()) and bool((raw == 0.5).all()) and bool((wav == 0.25).all())       # and nothing was written
    assert call(1, [8], [2], [16], [8], [16]) == 0 and _counter("ref_assess_launches") == 6 and _counter("ref_assess_clips") == 1
    torch.cuda.synchronize()
    assert int(rows[0, 0]) == 0 and bool((rows[1:] == -7).all())                 # a DC clip: clipped 0; the other rows are not the call's


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)
VOCAB = {chr(32 + i): i for i in range(96)}
REF_TEXT, TEXT = "Some call me nature", "I have been a silent spectator."


@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def _upload(seconds, seed, sr=24000, channels=1, clip_at=None):
    x = R.noisy_speech(int(seconds * R.RATE), seed)[1]
    if sr != R.RATE:
        n = int(seconds * sr)
        x = np.interp(np.arange(n) * (R.RATE / sr), np.arange(len(x)), x)
    if clip_at is not None:
        x = np.clip(x, -clip_at, clip_at) / clip_at
    return torch.from_numpy(np.stack([x * (1.0 - 0.1 * c) for c in range(channels)]).astype(np.float32)), sr


def test_prepare_voices_measures_the_flagged_voices_in_one_call(hip_objects):
    model, _ = hip_objects
    a, b, c = _upload(2.0, 31, 16000, 2, clip_at=0.2), _upload(1.5, 32, 16000), _upload(1.2, 33, 16000)
    today = model.prepare_voices([infer.PreparedVoice.deferred(a), infer.PreparedVoice.deferred(b), infer.PreparedVoice.deferred(c)])
    _reset()
    before = dict(infer.ASSESS_COUNTS)
    model.prepare_voices([infer.PreparedVoice.deferred(c)])
    assert _counter("ref_assess_launches") == 0 and dict(infer.ASSESS_COUNTS) == before              # nobody asked: nothing is measured
    va, vb, vc = infer.PreparedVoice.deferred(a, assess=True), infer.PreparedVoice.deferred(b, limits=dict(min_seconds=0.5)), infer.PreparedVoice.deferred(c)
    model.prepare_voices([va, vb, vc])
    assert _counter("ref_assess_launches") == 6 and _counter("ref_assess_clips") == 2                # two measured uploads, one not: ONE device call
    assert infer.ASSESS_COUNTS["device_calls"] == before.get("device_calls", 0) + 1 and infer.ASSESS_COUNTS["host_clips"] == before.get("host_clips", 0)
    assert vc.report is None
    for v, t, clip in ((va, today[0], a), (vb, today[1], b), (vc, today[2], c)):
        assert torch.equal(v.audio, t.audio) and torch.equal(v.mel, t.mel) and torch.equal(v.rms, t.rms)     # measuring changes nothing
    for v, t, clip in ((va, today[0], a), (vb, today[1], b)):
        want = audio_prep.assess_reference(clip[0].numpy(), clip[1], t.audio[0].cpu().numpy(), rms=float(t.rms))
        got = v.report
        print(f"[ref_assess] prepare_voices: device {got}\n[ref_assess] prepare_voices: host   {want}")
        assert (got.seconds, got.rms, got.peak, got.clipped, got.clip_ratio) == (want.seconds, want.rms, want.peak, want.clipped, want.clip_ratio)
        ref = reference_of(clip[0].numpy(), t.audio[0].cpu().numpy())
        assert abs(got.noise_db - ref["f64"]["noise_db"]) <= ref["bounds"]["noise_db"] and abs(got.snr_db - ref["f64"]["snr_db"]) <= ref["bounds"]["snr_db"]
        assert ref["near_bins"] == [] and got.bandwidth_hz == want.bandwidth_hz
        assert abs(got.speech_ratio - want.speech_ratio) * ref["f64"]["F"] <= len(ref["near_frames"]) + 1e-9
    assert va.report.clipped > 0
    gated = infer.PreparedVoice.deferred(a, limits=dict(max_clip_ratio=0.001))
    with pytest.raises(ValueError, match="clip_ratio is .* above the limit max_clip_ratio = 0.001"):
        model.prepare_voices([gated, infer.PreparedVoice.deferred(b)])
    assert gated.pending is not None


def _wav_bytes(clip):
    x, sr = clip
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(x.shape[0]); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(np.ascontiguousarray(infer.quantise_pcm16(x.numpy().T)).tobytes())
    return buf.getvalue()


def test_manager_refuses_a_clipped_upload_and_serves_a_clean_one_as_before(hip_objects, attn_shape_invariant):
    clipped, clean = _wav_bytes(_upload(1.6, 41, clip_at=0.08)), _wav_bytes(_upload(1.3, 42))
    plain = serve.TTSManager(nfe_step=4, device_frontend=True).load(*hip_objects)
    gated = serve.TTSManager(nfe_step=4, device_frontend=True, reference_limits=dict(max_clip_ratio=0.001, min_bandwidth_hz=6000.0)).load(*hip_objects)
    try:
        _reset()
        want = plain.synthesize_clip(TEXT, clean, REF_TEXT, seed=3)
        assert _counter("ref_assess_launches") == 0                              # no limits: nothing is measured
        with pytest.raises(ValueError, match="clip_ratio is .* above the limit max_clip_ratio = 0.001"):
            gated.synthesize_clip(TEXT, clipped, REF_TEXT, seed=3)
        assert _counter("ref_assess_launches") == 6 and len(gated._clip_cache) == 0 and _counter("ref_denoise_launches") == 0
        got = gated.synthesize_clip(TEXT, clean, REF_TEXT, seed=3)
        assert got.dtype == want.dtype and np.array_equal(got, want)             # byte for byte what it is without limits
        assert _counter("ref_assess_launches") == 12
        assert np.array_equal(gated.synthesize_clip(TEXT, clean, REF_TEXT, seed=3), want) and _counter("ref_assess_launches") == 12     # once per upload
        report = gated.check_reference(clean)
        assert report == gated._clip_voice(clean, REF_TEXT)[0].report and gated.reference_problems(report) == []
        assert "max_clip_ratio" in gated.reference_problems(gated.check_reference(clipped))[0]
    finally:
        plain.close()
        gated.close()
