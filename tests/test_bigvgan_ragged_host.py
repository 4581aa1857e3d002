"""CPU: `infer._chunk_waves` with mel_spec_type="bigvgan" hands every chunk of every group to ONE `decode_ragged` call when the vocoder object
offers the BigVGAN one (`ragged_mel_spec_type = "bigvgan"`, as F5HipBigVGAN does), and still calls any other vocoder chunk by chunk; the
waves are the same either way.  (The marker is there because tests/test_stream.py::test_bigvgan_keeps_the_per_chunk_loop pins that a bare
`decode_ragged`, which may be the Vocos kind, is never called on the BigVGAN path.)"""
import numpy as np
import torch

from tts_indic_server_f5_amd import infer

UP = 4
REF_FRAMES = 3
TARGET_RMS = 0.1


def _wave(spec):
    """stand-in generator: mel [C, T] -> wave [UP T]"""
    return spec.mean(dim=0).repeat_interleave(UP) * 0.01


class PerChunk:
    """what the reference's BigVGAN module offers: `vocoder(mel [1, C, T]) -> [1, 1, UP T]`"""

    def __init__(self):
        self.calls = []

    def __call__(self, mel):
        assert mel.dim() == 3 and mel.shape[0] == 1
        self.calls.append(("call", [tuple(mel.shape)]))
        return _wave(mel[0])[None, None]


class Ragged(PerChunk):
    ragged_mel_spec_type = "bigvgan"

    def decode_ragged(self, mels):
        assert all(m.dim() == 2 for m in mels)
        self.calls.append(("ragged", [m.clone() for m in mels]))
        return [_wave(m) for m in mels]


def _groups():
    g = torch.Generator().manual_seed(4)
    lens = [[9, 14], [7, 21, 5]]
    rms = [0.2, 0.04]   # the second voice is below target_rms: its chunks are scaled back by rms / target_rms
    return [([torch.randn(REF_FRAMES + t, 100, generator=g) for t in ts], REF_FRAMES, r) for ts, r in zip(lens, rms)], lens, rms


def test_one_decode_ragged_call_for_all_groups():
    groups, lens, rms = _groups()
    voc = Ragged()
    out = infer._chunk_waves(groups, voc, "bigvgan", TARGET_RMS)
    assert [kind for kind, _ in voc.calls] == ["ragged"]
    items = voc.calls[0][1]
    want = [mel[REF_FRAMES:].t() for mels, _, _ in groups for mel in mels]   # group order, reference frames stripped
    assert len(items) == 5 and all(torch.equal(a, b) for a, b in zip(items, want))

    loop_voc = PerChunk()
    loop = infer._chunk_waves(groups, loop_voc, "bigvgan", TARGET_RMS)
    assert [kind for kind, _ in loop_voc.calls] == ["call"] * 5
    assert [shape for _, (shape,) in loop_voc.calls] == [(1, 100, t) for ts in lens for t in ts]

    for (waves, specs), (waves1, specs1), ts, r, (mels, _, _) in zip(out, loop, lens, rms, groups):
        assert len(waves) == len(waves1) == len(ts)
        for w, w1, s, s1, t, mel in zip(waves, waves1, specs, specs1, ts, mels):
            assert isinstance(w, np.ndarray) and w.shape == w1.shape == (UP * t,) and w.dtype == w1.dtype == np.float32
            np.testing.assert_array_equal(w, w1)
            np.testing.assert_array_equal(s, s1)
            ref = _wave(mel[REF_FRAMES:].t())
            if r < TARGET_RMS:
                ref = ref * r / TARGET_RMS
            np.testing.assert_array_equal(w, ref.numpy())


def test_no_chunks_means_no_vocoder_call():
    voc = Ragged()
    assert infer._chunk_waves([([], REF_FRAMES, 0.2)], voc, "bigvgan", TARGET_RMS) == [([], [])]
    assert voc.calls == []


def test_a_bare_decode_ragged_is_not_called_for_bigvgan():
    class VocosStyle(PerChunk):
        def decode_ragged(self, mels):
            raise AssertionError("a decode_ragged that does not declare itself BigVGAN's")

    groups, lens, _ = _groups()
    voc = VocosStyle()
    infer._chunk_waves(groups, voc, "bigvgan", TARGET_RMS)
    assert [kind for kind, _ in voc.calls] == ["call"] * 5


def test_a_single_bigvgan_chunk_takes_the_plain_forward():
    g = torch.Generator().manual_seed(5)
    voc = Ragged()
    (waves, specs), = infer._chunk_waves([([torch.randn(REF_FRAMES + 6, 100, generator=g)], REF_FRAMES, 0.2)], voc, "bigvgan", TARGET_RMS)
    assert [kind for kind, _ in voc.calls] == ["call"] and waves[0].shape == (UP * 6,)
