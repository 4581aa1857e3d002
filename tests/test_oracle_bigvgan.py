"""CPU known-answer tests for the BigVGAN restatement (third-party, parity unpinned by the reference): SURVEY C.3."""
import torch

from oracle import bigvgan_oracle as B
from tts_indic_server_f5_amd import synth

SMALL = dict(upsample_initial_channel=64)


def test_aa_filter_dc_gain_and_symmetry():
    f = B.aa_filter()
    assert f.shape == (12,) and abs(float(f.sum()) - 1.0) < 1e-6
    assert torch.allclose(f, f.flip(0), atol=1e-7)


def test_up_down_length_and_dc():
    x = torch.full((1, 3, 40), 0.7)
    u = B.upsample2(x)
    assert u.shape == (1, 3, 80) and torch.allclose(u, torch.full_like(u, 0.7), atol=1e-5)   # DC gain 1 incl. the x2
    d = B.downsample2(u)
    assert d.shape == (1, 3, 40) and torch.allclose(d, x, atol=1e-5)


def test_snake_beta_identity_points():
    x = torch.zeros(1, 4, 8)
    assert torch.equal(B.snake_beta(x, torch.zeros(4), torch.zeros(4)), x)
    y = B.snake_beta(torch.full((1, 1, 1), math_pi_half()), torch.zeros(1), torch.zeros(1))
    assert abs(float(y) - (math_pi_half() + 1.0)) < 1e-5     # x + sin^2(x) / 1


def math_pi_half():
    import math
    return math.pi / 2


def test_forward_length_and_range():
    cfg = B.BigVGANConfig(upsample_initial_channel=64)
    sd = synth.bigvgan_state_dict(**SMALL)
    mel = torch.randn(2, 100, 9)
    w = B.bigvgan_forward(sd, cfg, mel)
    assert w.shape == (2, 1, 9 * 256) and torch.isfinite(w).all() and w.abs().max() <= 1.0
    assert w.std() > 1e-3


def test_bigvgan_mel_shape():
    wave = synth.ref_audio(24000)
    m = B.bigvgan_mel_spectrogram(wave)
    assert m.shape == (1, 100, 24000 // 256) and torch.isfinite(m).all()
    fb = B.librosa_slaney_mel(24000, 1024, 100)
    assert fb.shape == (100, 513) and (fb >= 0).all() and (fb.sum(1) > 0).all()


def _fp32_filter_as_before():
    """The fp32 filter as the oracle built it before it followed its input's dtype: window and time grid in torch's default dtype."""
    import math
    half, A = 6, 2.285 * 5 * math.pi * 1.2 + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50.0 else (0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21.0 else 0.0)
    window = torch.kaiser_window(12, beta=beta, periodic=False)
    filt = 2 * 0.25 * window * torch.sinc(2 * 0.25 * (torch.arange(-half, half) + 0.5))
    return filt / filt.sum()


def test_oracle_dtype_follows_input():
    """fp32 calls are bit-identical to the fp32-only oracle (same filter bits, same operator chain); float64 inputs give a float64 path
    whose filter agrees with the fp32 one to fp32 rounding, and a float64 forward that agrees with the fp32 forward to fp32 accuracy."""
    import torch.nn.functional as F
    old = _fp32_filter_as_before()
    assert B.aa_filter().dtype == torch.float32 and torch.equal(B.aa_filter(), old)
    f64 = B.aa_filter(torch.float64)
    assert f64.dtype == torch.float64 and abs(float(f64.sum()) - 1.0) < 1e-14
    assert (f64 - old.double()).abs().max() < 1e-7
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 5, 37, generator=g) * 3
    al, be = torch.randn(5, generator=g), torch.randn(5, generator=g)
    up_old = (2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), old.view(1, 1, 12).expand(5, -1, -1), stride=2, groups=5))[..., 15:-15]
    assert torch.equal(B.upsample2(x), up_old)
    down_old = F.conv1d(F.pad(up_old, (5, 6), mode="replicate"), old.view(1, 1, 12).expand(5, -1, -1), stride=2, groups=5)
    assert torch.equal(B.downsample2(up_old), down_old)
    assert torch.equal(B.activation1d(x, al, be), B.downsample2(B.snake_beta(up_old, al, be)))
    y64 = B.activation1d(x.double(), al.double(), be.double())
    assert y64.dtype == torch.float64 and (y64 - B.activation1d(x, al, be).double()).abs().max() < 1e-4
    cfg = B.BigVGANConfig(upsample_initial_channel=32, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4))
    sd = synth.bigvgan_state_dict(upsample_initial_channel=32, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4))
    mel = torch.randn(1, 100, 6, generator=g)
    w32 = B.bigvgan_forward(sd, cfg, mel)
    w64 = B.bigvgan_forward({k: v.double() for k, v in sd.items()}, cfg, mel.double())
    assert w32.dtype == torch.float32 and w64.dtype == torch.float64 and w64.shape == w32.shape == (1, 1, 48)
    assert (w64 - w32.double()).abs().max() < 1e-5


def test_snake_scale_default_keeps_weights():
    """synth.bigvgan_state_dict(snake_scale=None) is the historical draw; a scale rescales only the SnakeBeta log-parameters."""
    arch = dict(upsample_initial_channel=32, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4))
    a = synth.make_state_dict(synth.bigvgan_param_specs(**arch), synth.SEED_BIGVGAN)
    b = synth.bigvgan_state_dict(**arch)
    c = synth.bigvgan_state_dict(snake_scale=1.0, **arch)
    assert a.keys() == b.keys() == c.keys()
    for k in a:
        assert torch.equal(a[k], b[k])
        snake = k.endswith(".act.alpha") or k.endswith(".act.beta")
        assert torch.equal(c[k], a[k] * 5.0) if snake else torch.equal(c[k], a[k])
