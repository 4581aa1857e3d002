"""The device front-end for reference audio (csrc/resample.h, f5hip_ref_frontend: mono mix, rms, gain, polyphase sinc resampling of a
ragged batch of clips in two launches) against an fp64 restatement, then `infer.prepare_voices` against the host `_prepare_reference`, and
`TTSManager.synthesize_clip` end to end on a tiny model.

Bounds (derived, not tuned): per output sample |y - y64| <= (L + 4) * 2^-24 * sum_k |taps_k * x_k| with L the taps per phase -- the fp32
dot-product bound plus the two roundings of the gain, the one of the mono mean (fp64 sum, rounded once) and the rms's; rms within 2^-22 relative (fp64 accumulation, one rounding, one sqrt).
Every signal is scaled so that its mono rms IS the stated amplitude (0.3: no gain, 0.02: gain) whatever its length, so the rms < 0.1 branch
cannot flip on rounding."""
import ctypes as C
import io
import math
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, ops, synth  # noqa: E402

RATES = [48000, 16000, 44100, 22050, 11025]          # -> 24 000: trivial table, up-sampling, the large table in LDS (x2), the one beyond LDS
FLOOR = float(np.float32(0.1))                       # the rms floor as the kernel receives it
EPS = 2.0 ** -24


def _pair(sr):
    g = math.gcd(sr, 24000)
    return sr // g, 24000 // g


def _lengths(sr):
    of = _pair(sr)[0] if sr != 24000 else 7
    return [1, 5, max(of - 1, 1), of, of + 1, 3 * of + 1, 4411]


def _clip(n, ch, amp, seed):
    """fp32 [ch, n] whose mono mean has rms `amp` (to fp32 rounding)"""
    x = np.random.default_rng(seed).standard_normal((ch, n))
    m = x.mean(0)
    return (x * (amp / math.sqrt(float(np.mean(m * m))))).astype(np.float32)


def _ref64(x, sr):
    """(y64, sum_k |taps_k x_k|, rms64, L) of one clip: mono mean, rms, gain, resampling, all in fp64 on the fp32 inputs and fp32 tap values"""
    m = x.astype(np.float64).mean(0)
    rms = math.sqrt(float(np.mean(m * m)))
    g = m * FLOOR / rms if rms < FLOOR else m
    if sr == 24000:
        return g, np.abs(g), rms, 0
    of, nf, width, taps = infer.resample_taps(sr, 24000)
    t64 = taps.numpy().astype(np.float64)
    L = t64.shape[1]
    xpad = np.concatenate([np.zeros(width), g, np.zeros(width + of)])
    j = np.arange(-(-nf * len(g) // of))
    q, p = j // nf, j % nf
    prod = t64[p] * xpad[q[:, None] * of + np.arange(L)[None, :]]
    return prod.sum(1), np.abs(prod).sum(1), rms, L


def _run(clips, sr):
    """ops.ref_frontend on the clips [ch_i, n_i] packed back to back -> ([y_i] numpy, rms numpy)"""
    dev = torch.device("cuda:0")
    packed = torch.from_numpy(np.concatenate([c.reshape(-1) for c in clips])).to(dev)
    taps = None if sr == 24000 else infer.resample_taps(sr, 24000)[3].to(dev)
    out, rms, n_out = ops.ref_frontend(packed, [c.shape[1] for c in clips], [c.shape[0] for c in clips], sr, 24000, taps, FLOOR)
    return [o.cpu().numpy() for o in out.split(n_out)], rms.cpu().numpy()


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _check(y, rms, x, sr, tag):
    y64, mag, rms64, L = _ref64(x, sr)
    assert y.shape == y64.shape, tag
    assert np.isfinite(y).all(), tag
    excess = np.abs(y.astype(np.float64) - y64) - (L + 4) * EPS * mag
    rel = abs(float(rms) - rms64) / rms64
    print(f"[ref_frontend] {tag}: worst |err| / bound {float(np.max(np.abs(y - y64) / np.maximum((L + 4) * EPS * mag, 1e-300))):.3f}  rms rel err {rel:.2e}")
    assert (excess <= 0).all(), (tag, float(excess.max()))
    assert rel <= 2.0 ** -22, (tag, rel)


@pytest.mark.parametrize("amp", [0.3, 0.02])
@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("sr", RATES + [24000])
def test_each_clip_within_the_fp32_bound_of_fp64(sr, ch, amp):
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")
    lengths = _lengths(sr)
    for i, n in enumerate(lengths):
        x = _clip(n, ch, amp, seed=1000 * ch + i)
        (y,), rms = _run([x], sr)
        _check(y, rms[0], x, sr, f"{sr} Hz, {ch} ch, amp {amp}, n {n}")
    assert _counter("ref_frontend_launches") == 2 * len(lengths)          # two launches per call
    if sr != 24000:   # the table is staged in LDS when it fits a CU's 160 KB next to the input window, else read through L2
        of, nf, width, _ = infer.resample_taps(sr, 24000)
        in_lds = 4 * nf * (2 * width + of) < 150 * 1024
        assert in_lds == (sr != 11025)
        assert (_counter("ref_taps_lds"), _counter("ref_taps_l2")) == ((len(lengths), 0) if in_lds else (0, len(lengths)))


def test_identity_keeps_the_bits():
    x = _clip(4411, 1, 0.3, seed=3)
    (y,), rms = _run([x], 24000)
    assert np.array_equal(y.view(np.uint32), x[0].view(np.uint32))
    assert abs(float(rms[0]) - 0.3) < 1e-6


@pytest.mark.parametrize("sr", RATES + [24000])
def test_a_clip_in_a_batch_equals_its_own_call(sr):
    """All seven lengths in one call, in two orders, mixed channel counts and both gain branches: samples and rms equal each clip's own
    call bit for bit (the neighbours in the packed buffer are other clips' samples, so a read across a clip's edge shows here)."""
    clips = [_clip(n, 1 + i % 3, 0.3 if i % 2 else 0.02, seed=50 + i) for i, n in enumerate(_lengths(sr))]
    solo = [_run([c], sr) for c in clips]
    for order in (list(range(len(clips))), [3, 6, 0, 5, 1, 4, 2]):
        ys, rms = _run([clips[i] for i in order], sr)
        for k, i in enumerate(order):
            assert np.array_equal(ys[k].view(np.uint32), solo[i][0][0].view(np.uint32)), (sr, order, i)
            assert rms[k:k + 1].view(np.uint32) == solo[i][1].view(np.uint32), (sr, order, i)


def test_ctypes_and_torch_op_paths_agree():
    """`ops.ref_frontend` through the TORCH_LIBRARY operator and through ctypes: the same C entry point, so the same bits.  One call of a mono
    clip of 3 001 samples and a stereo clip of 1 777 at 44 100 -> 24 000 Hz: odd lengths that are no multiple of the 147-sample polyphase
    period, so the ragged tail and the channel mix are both exercised."""
    from tts_indic_server_f5_amd import torch_ops
    dev = torch.device("cuda:0")
    clips = [_clip(3001, 1, 0.3, seed=71), _clip(1777, 2, 0.02, seed=72)]
    packed = torch.from_numpy(np.concatenate([c.reshape(-1) for c in clips])).to(dev)
    taps = infer.resample_taps(44100, 24000)[3].to(dev)
    run = lambda: ops.ref_frontend(packed, [3001, 1777], [1, 2], 44100, 24000, taps, FLOOR)   # noqa: E731
    out, rms, n_out = run()
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        out2, rms2, n_out2 = run()
    finally:
        torch_ops._loaded = True
    assert n_out == n_out2 == [-(-3001 * 80 // 147), -(-1777 * 80 // 147)] and out.numel() == sum(n_out)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(rms.view(torch.int32), rms2.view(torch.int32))


def test_refusals_come_before_any_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    wave_dev, out, rms = torch.zeros(64, device=dev), torch.zeros(64, device=dev), torch.zeros(4, device=dev)
    taps = infer.resample_taps(48000, 24000)[3].to(dev)

    def call(n, n_in, ch, orig, new, taps_ptr):
        a, b = np.asarray(n_in, dtype=np.int32), np.asarray(ch, dtype=np.int32)
        return lib.f5hip_ref_frontend(n, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(wave_dev.data_ptr()), orig, new, taps_ptr,
                                      C.c_float(FLOOR), C.c_void_p(out.data_ptr()), C.c_void_p(rms.data_ptr()), _lib.current_stream_ptr())

    tp = C.c_void_p(taps.data_ptr())
    _lib.check(lib.f5hip_get_counter(b"reset", None), "reset counters")
    assert call(0, [8], [1], 48000, 24000, tp) != 0                      # n < 1
    assert call(2, [8, 0], [1, 1], 48000, 24000, tp) != 0                # n_in[i] < 1
    assert call(2, [8, 8], [1, 0], 48000, 24000, tp) != 0                # channels[i] < 1
    assert call(1, [8], [1], 48000, 24000, None) != 0                    # no table although the rates differ
    assert call(2, [2 ** 31 - 1, 2 ** 31 - 1], [1, 1], 24000, 24000, None) != 0    # sum(n_out) overflows int32
    assert lib.f5hip_last_error()
    # a table of another shape (another lowpass_filter_width) would be read with the wrong stride: the wrapper and the operator refuse it
    wide = infer.resample_taps(48000, 24000, lowpass_filter_width=8)[3].to(dev)
    with pytest.raises(_lib.F5HipError, match="taps must be"):
        ops.ref_frontend(wave_dev[:8], [8], [1], 48000, 24000, wide, FLOOR)
    with pytest.raises(RuntimeError, match="taps must be"):
        torch.ops.f5hip.ref_frontend(wave_dev[:8], torch.tensor([8], dtype=torch.int32), torch.tensor([1], dtype=torch.int32), 48000, 24000, wide, FLOOR)
    assert _counter("ref_frontend_launches") == 0
    assert call(1, [8], [1], 24000, 24000, None) == 0 and _counter("ref_frontend_launches") == 2
    torch.cuda.synchronize()


def test_prepare_voices_matches_the_host_front_end():
    """Three clips at two rates: one upload and one call per rate.  audio within the per-sample bound of the host path, ref_frames / seconds equal, rms within 2^-22, the mel from cond() within the project's mel bound
    (1e-3 rms) of the host path's mel."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    arch = dict(dim=256, depth=2, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=40)
    model = F5HipModel(DiTArch(**arch), synth.dit_state_dict(**arch))
    clips = [(torch.from_numpy(_clip(30011, 2, 0.3, seed=1)), 44100), (torch.from_numpy(_clip(26000, 1, 0.02, seed=2)), 48000),
             (torch.from_numpy(_clip(20000, 3, 0.02, seed=3)), 44100)]
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")
    voices = infer.prepare_voices(clips, target_rms=0.1, device="cuda:0")
    assert _counter("ref_frontend_launches") == 4                         # two rates, two launches each
    for (wav, sr), v in zip(clips, voices):
        host = infer.PreparedVoice((wav, sr), 0.1)
        assert v.pending is None and v.audio.is_cuda and v.audio.shape == host.audio.shape
        assert v.ref_frames == host.ref_frames and v.seconds == host.seconds
        _, mag, _, L = _ref64(wav.numpy(), sr)
        d = np.abs(v.audio[0].cpu().numpy().astype(np.float64) - host.audio[0].numpy().astype(np.float64))
        assert (d <= (L + 4) * EPS * mag).all(), float((d - (L + 4) * EPS * mag).max())
        assert abs(float(v.rms) - float(host.rms)) / float(host.rms) <= 2.0 ** -22
        mel_err = float((v.cond(model) - host.cond(model)).pow(2).mean().sqrt())
        print(f"[ref_frontend] prepare_voices {sr} Hz x {wav.shape[0]} ch: mel rms vs host front-end {mel_err:.3e}")
        assert mel_err < 1e-3


# ------------------------------------------------------------------------------------------------ end to end on a tiny model
ARCH = dict(dim=256, depth=4, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=96)
VOCAB = {chr(32 + i): i for i in range(96)}
REF_TEXT, TEXT = "Some call me nature", "I have been a silent spectator. Always remember, I endure."


def _wav_bytes(x, sr):
    """16-bit PCM WAV of x [ch, n] float"""
    buf = io.BytesIO()
    with wave.open(buf, "wb") as f:
        f.setnchannels(x.shape[0]); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes(np.clip(np.rint(x.T * 32768), -32768, 32767).astype("<i2").tobytes())
    return buf.getvalue()


@pytest.fixture(scope="module")
def hip_objects():
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    return F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB), F5HipVocos(synth.vocos_state_dict())


def _tone(n, sr, seed, amp):
    """speech-like test signal at any rate: synth.ref_audio is defined per sample, so it is drawn at 24 kHz length and reused as is"""
    return synth.ref_audio(n, seed=seed, amp=amp)[0].numpy()


def test_synthesize_clip_equals_a_registered_voice_at_24k(hip_objects, tmp_path):
    """24 kHz mono 16-bit at rms >= 0.1: the front-end is the identity there, so the uploaded clip and the same file as a registered voice
    give the same wave bit for bit, on the device front-end and on the host one."""
    from tts_indic_server_f5_amd import serve
    x = np.concatenate([np.zeros(4800), _tone(24000 * 2, 24000, 0, 0.3), np.zeros(2400)])[None]
    assert math.sqrt(float(np.mean(x ** 2))) >= 0.1 and np.abs(x).max() < 1.0
    raw = _wav_bytes(x, 24000)
    path = tmp_path / "voice.wav"
    path.write_bytes(raw)
    for device_frontend in (True, False):
        mgr = serve.TTSManager(nfe_step=8, device_frontend=device_frontend).load(*hip_objects)
        want = mgr.synthesize(TEXT, ref_audio_path=str(path), ref_text=REF_TEXT, seed=11)
        got = mgr.synthesize_clip(TEXT, raw, REF_TEXT, seed=11)
        assert got.shape == want.shape and np.array_equal(got, want), device_frontend


def test_synthesize_clip_device_front_end_vs_host_front_end_at_44k(hip_objects):
    from tts_indic_server_f5_amd import serve
    a, b = _tone(int(44100 * 2.2), 44100, 1, 0.12), _tone(int(44100 * 2.2), 44100, 2, 0.12)
    raw = _wav_bytes(np.stack([a, 0.5 * a + 0.5 * b]), 44100)
    waves = []
    for device_frontend in (True, False):
        mgr = serve.TTSManager(nfe_step=8, device_frontend=device_frontend).load(*hip_objects)
        _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")
        waves.append(mgr.synthesize_clip(TEXT, raw, REF_TEXT, seed=5))
        assert _counter("ref_frontend_launches") == (2 if device_frontend else 0)      # the device front-end ran, resp. did not
    # the comparison means something only if the wave depends on the clip: the same upload, 1e-3 louder, gives another wave
    louder = mgr.synthesize_clip(TEXT, _wav_bytes(np.stack([a, 0.5 * a + 0.5 * b]) * 1.001 + 1e-3, 44100), REF_TEXT, seed=5)
    assert louder.shape == waves[1].shape and float(np.abs(louder - waves[1]).max()) > 1e-5
    err = float(np.abs(waves[0] - waves[1]).max())
    print(f"[ref_frontend] synthesize_clip 44.1 kHz stereo: wave max |device front-end - host front-end| {err:.3e} (n = {len(waves[0])})")
    assert waves[0].shape == waves[1].shape and err < 1e-4


def test_uploads_and_a_registered_voice_share_a_batch(hip_objects):
    """Two uploads (deferred voices: one ragged front-end call) and one eager voice in one `infer_requests` batch: each equals its solo result
    bit for bit."""
    model, voc = hip_objects
    model.set_attention_shape_invariant(True)
    try:
        a = torch.from_numpy(np.stack([_tone(50000, 44100, 4, 0.05), _tone(50000, 44100, 5, 0.05)]).astype(np.float32))
        b = torch.from_numpy(_tone(41000, 44100, 6, 0.2)[None].astype(np.float32))
        c = (synth.ref_audio(24000 * 2, amp=0.15), 24000)

        def requests():
            return [(infer.PreparedVoice.deferred((a, 44100)), "Some call me nature.", TEXT, dict(seed=1)),
                    (infer.PreparedVoice.deferred((b, 44100)), "Others say mother.", "Always remember, I endure.", dict(seed=2)),
                    (infer.PreparedVoice(c), "Some call me nature.", "Short.", dict(seed=3))]
        _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")
        batch = infer.infer_requests(requests(), model, voc, nfe_step=8)
        assert _counter("ref_frontend_launches") == 2                     # both uploads in one call
        solo = [infer.infer_requests([r], model, voc, nfe_step=8)[0] for r in requests()]
        for (w, _, s), (w1, _, s1) in zip(batch, solo):
            assert np.array_equal(w, w1) and np.array_equal(s, s1)
    finally:
        model.set_attention_shape_invariant(False)
