"""The ragged reference mel (csrc/vocos.h, f5hip_mel_spectrogram_ragged: both mel front-ends for several clips of their own lengths in one
launch, frame-major and packed) against `F5HipModel.cond_mel` of each clip alone, and `F5HipModel.prepare_voices`, which fills the mels of a
batch's new voices with it.  Every comparison is `torch.equal`: there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import _lib, infer, mel, synth, torch_ops  # noqa: E402
from tts_indic_server_f5_amd.model import DiTArch, F5HipModel  # noqa: E402

ARCH = dict(dim=256, depth=2, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=40)
VARIANTS = ["vocos", "bigvgan"]
# around the reflect pad (513: vocos' shortest clip; 1024: bigvgan's) and around a frame boundary (1280 = 5 hops), then one second
LENGTHS = {"vocos": [513, 1024, 1279, 1280, 1281, 24000], "bigvgan": [1024, 1279, 1280, 1281, 24000]}


def _counter(name):
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _clip(n, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def models():
    sd = synth.dit_state_dict(**ARCH)
    return {v: F5HipModel(DiTArch(**ARCH), sd, mel_spec_type=v) for v in VARIANTS}


@pytest.fixture(scope="module")
def alone(models):
    """{variant: [cond_mel(clip)[0] per length]}: each clip through the single-clip front-end, computed once and shared"""
    dev = torch.device("cuda:0")
    return {v: [models[v].cond_mel(torch.from_numpy(_clip(n, 10 + i))[None].to(dev))[0].clone() for i, n in enumerate(LENGTHS[v])] for v in VARIANTS}


def _device(clips, variant, packed):
    """mel_spectrogram_ragged on device copies -> [rows per clip].  `packed`: the clips are views of ONE buffer, back to back like
    `ref_frontend` leaves them; else separate allocations with a loud filler around each (a read across a clip's end would show)."""
    dev = torch.device("cuda:0")
    if packed:
        waves = list(torch.from_numpy(np.concatenate(clips)).to(dev).split([len(c) for c in clips]))
    else:
        waves = []
        for c in clips:
            buf = torch.full((len(c) + 2048,), 50.0, device=dev)
            buf[1024:1024 + len(c)] = torch.from_numpy(c).to(dev)
            waves.append(buf[1024:1024 + len(c)])
    out, frames = mel.mel_spectrogram_ragged(waves, variant)
    assert out.shape == (sum(frames), 100) and out.is_contiguous()
    assert frames == [mel.mel_frames(len(c), variant) for c in clips]
    return list(out.split(frames))


@pytest.mark.parametrize("variant", VARIANTS)
def test_item_rows_equal_cond_mel_of_the_clip_alone(models, alone, variant):
    lens = LENGTHS[variant]
    clips = [_clip(n, 10 + i) for i, n in enumerate(lens)]
    deals = [list(range(len(lens)))] + [[0], [1, 2], [3, 4, 5][:len(lens) - 3]]          # all in one call, then calls of 1 to 3
    for deal in deals:
        for packed in (True, False):
            _reset()
            got = _device([clips[i] for i in deal], variant, packed)
            assert _counter("mel_ragged_launches") == 1 and _counter("mel_ragged_items") == len(deal)      # one launch whatever n
            for i, g in zip(deal, got):
                w = alone[variant][i]
                assert g.shape == w.shape, (variant, lens[i], tuple(g.shape), tuple(w.shape))
                assert torch.equal(g, w), (variant, lens[i], packed, float((g - w).abs().max()))
    # the model's own call: views [1, T, mel] of one packed buffer
    dev = torch.device("cuda:0")
    mels = models[variant].cond_mel_ragged([torch.from_numpy(c)[None].to(dev) for c in clips])
    assert all(m.shape == (1,) + tuple(w.shape) and torch.equal(m[0], w) for m, w in zip(mels, alone[variant]))
    # a neighbour's loudness does not reach a clip: the same clip between two others, packed
    a, b = _device([clips[1]], variant, True)[0], _device([50 * clips[2], clips[1], 50 * clips[3]], variant, True)[1]
    assert torch.equal(a, b)


def test_ctypes_and_torch_op_paths_agree(alone):
    clips = [_clip(n, 10 + i) for i, n in enumerate(LENGTHS["vocos"])]
    assert torch_ops.load()
    try:
        torch_ops._loaded = False                      # force the ctypes binding
        got = _device(clips, "vocos", True)
    finally:
        torch_ops._loaded = True
    assert all(torch.equal(g, w) for g, w in zip(got, alone["vocos"]))
    dev = torch.device("cuda:0")
    out = torch.ops.f5hip.mel_spectrogram_ragged([torch.from_numpy(c).to(dev) for c in clips], 1024, 256, 100, 24000, 0)
    assert torch.equal(out, torch.cat(alone["vocos"]))


def test_refusals_come_before_the_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    wave = torch.zeros(4096, device=dev)
    out = torch.zeros(64 * 100, device=dev)

    def call(lens, variant=0, n=None, ptr=None, n_fft=1024, hop=256, n_mels=100, out_p=out.data_ptr(), lens_p=True, ptrs_p=True):
        ls = np.asarray(lens, dtype=np.int32)
        ptrs = np.full(len(ls), wave.data_ptr() if ptr is None else ptr, dtype=np.uint64)
        return lib.f5hip_mel_spectrogram_ragged(len(ls) if n is None else n, C.c_void_p(ls.ctypes.data) if lens_p else None,
                                                C.c_void_p(ptrs.ctypes.data) if ptrs_p else None, C.c_void_p(out_p), n_fft, hop, n_mels, 24000, variant,
                                                _lib.current_stream_ptr())

    _reset()
    assert call([1024, 512]) != 0 and b"clip 1" in lib.f5hip_last_error()                  # vocos: n_samples > n_fft / 2
    assert call([1024, 1023], variant=1) != 0 and b"clip 1" in lib.f5hip_last_error()      # bigvgan: n_samples >= n_fft
    assert call([1024], variant=2) != 0 and b"variant" in lib.f5hip_last_error()
    assert call([1024], n=0) != 0 and call([], n=0) != 0 and call([1024], ptr=0) != 0
    assert call([1024], out_p=None) != 0 and call([1024], lens_p=False) != 0 and call([1024], ptrs_p=False) != 0
    assert call([1024], n_fft=512) != 0 and call([1024], hop=0) != 0 and call([1024], n_mels=0) != 0 and call([1024], n_mels=257) != 0
    with pytest.raises(_lib.F5HipError, match="clip 1"):
        mel.mel_spectrogram_ragged([wave[:1024], wave[1024:1536]], "vocos")
    with pytest.raises(_lib.F5HipError, match="clip 0"):
        mel.mel_spectrogram_ragged([wave[:1023]], "bigvgan")
    with pytest.raises(_lib.F5HipError, match="variant"):
        mel.mel_spectrogram_ragged([wave[:1024]], "slaney")
    with pytest.raises(_lib.F5HipError):
        mel.mel_spectrogram_ragged([], "vocos")
    with pytest.raises(_lib.F5HipError):
        mel.mel_spectrogram_ragged([wave[:1024].cpu()], "vocos")
    with pytest.raises(RuntimeError, match="clip 0"):
        torch.ops.f5hip.mel_spectrogram_ragged([wave[:512]], 1024, 256, 100, 24000, 0)
    with pytest.raises(RuntimeError, match="variant"):
        torch.ops.f5hip.mel_spectrogram_ragged([wave[:1024]], 1024, 256, 100, 24000, 2)
    assert _counter("mel_ragged_launches") == 0 and _counter("mel_ragged_items") == 0
    assert call([513, 1024]) == 0 and _counter("mel_ragged_launches") == 1 and _counter("mel_ragged_items") == 2
    torch.cuda.synchronize()


def test_prepare_voices_fills_the_mels_in_one_launch(models):
    """Three uploaded clips of two source rates: `F5HipModel.prepare_voices` makes one mel launch and fills three mels equal to the lazy ones;
    a deferred voice has no mel until it is prepared, and a voice that is already prepared is left alone."""
    model = models["vocos"]
    clip = lambda n, ch, seed: torch.from_numpy((0.1 * np.random.default_rng(seed).standard_normal((ch, n))).astype(np.float32))   # noqa: E731
    clips = [(clip(30011, 2, 1), 44100), (clip(26000, 1, 2), 48000), (clip(20000, 3, 3), 44100)]
    voices = [infer.PreparedVoice.deferred(c) for c in clips]
    assert all(v.mel is None and v.pending is not None for v in voices)
    _reset()
    model.prepare_voices(voices)
    assert _counter("mel_ragged_launches") == 1 and _counter("mel_ragged_items") == 3
    assert _counter("ref_frontend_launches") == 4                          # two rates, two launches each: as before
    for v in voices:
        assert v.pending is None and v.mel is not None and v.mel.shape[0] == 1 and v.mel.shape[2] == 100
        lazy = model.cond_mel(v.audio)
        assert torch.equal(v.mel, lazy) and v.cond(model) is v.mel
    _reset()
    model.prepare_voices(voices)                                           # nothing is pending: nothing runs
    late = infer.PreparedVoice.deferred(clips[1])
    kept = voices[0].mel
    model.prepare_voices([voices[0], late])
    assert _counter("mel_ragged_launches") == 1 and _counter("mel_ragged_items") == 1 and voices[0].mel is kept
    assert torch.equal(late.mel, voices[1].mel)
