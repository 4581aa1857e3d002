"""GPU parity (through the C ABI) of the BigVGAN v2 generator and its mel front-end vs the CPU oracle
(third-party leaf, parity unpinned by the reference).  Tolerance: 1e-4 on waveform samples (BASELINE north_star)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mel_ref import bigvgan_mel_float64 as _mel_float64  # noqa: E402
from oracle import bigvgan_oracle as B  # noqa: E402
from tts_indic_server_f5_amd import synth  # noqa: E402


def _report(tag, got, ref):
    d = got.float().cpu() - ref.float().cpu()
    print(f"[parity] {tag}: rms_err {d.pow(2).mean().sqrt():.3e} max_err {d.abs().max():.3e} ref_rms {ref.float().pow(2).mean().sqrt():.3e}")
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("b,t", [(1, 40), (2, 13), (1, 130)])
def test_bigvgan_small_config(b, t):
    """Reduced-width generator (initial channel 256 -> 128 ... 4): every stage incl. the padded-channel tail."""
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    sd = synth.bigvgan_state_dict(upsample_initial_channel=256)
    voc = F5HipBigVGAN(sd, upsample_initial_channel=256)
    g = torch.Generator().manual_seed(200 + t)
    mel = torch.randn(b, 100, t, generator=g) * 1.5 - 1.0
    ref = B.bigvgan_forward(sd, B.BigVGANConfig(upsample_initial_channel=256), mel)
    got = voc(mel)
    assert got.shape == ref.shape == (b, 1, 256 * t)
    mx, rms = _report(f"bigvgan c0=256 b{b} t{t}", got, ref)
    assert mx < 1e-4


@pytest.mark.parametrize("b,t", [(1, 40), (2, 13)])
def test_bigvgan_small_config_fp16_fast_mode(b, t):
    """gemm_planes=3 (one fp16 operand plane: a third of the MFMA work).  NOT a parity mode: 11-bit operands through 36 residual
    convolutions per stage measure ~1e-3 max / 2e-4 rms on the waveform (tools/bigvgan_modes.py), ten times the 1e-4 bound that
    the default split-bf16 mode meets; the bound asserted here is that measured level with 2x head room, so a regression shows."""
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    sd = synth.bigvgan_state_dict(upsample_initial_channel=256)
    voc = F5HipBigVGAN(sd, upsample_initial_channel=256, gemm_planes=3)
    g = torch.Generator().manual_seed(200 + t)
    mel = torch.randn(b, 100, t, generator=g) * 1.5 - 1.0
    ref = B.bigvgan_forward(sd, B.BigVGANConfig(upsample_initial_channel=256), mel)
    mx, rms = _report(f"bigvgan fp16 fast mode c0=256 b{b} t{t}", voc(mel), ref)
    assert mx < 2.5e-3 and rms < 5e-4


def test_bigvgan_full_config():
    """bigvgan_v2_24khz_100band_256x geometry (112 M parameters), 48 frames."""
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    sd = synth.bigvgan_state_dict()
    voc = F5HipBigVGAN(sd)
    g = torch.Generator().manual_seed(77)
    mel = torch.randn(1, 100, 48, generator=g) * 1.5 - 1.0
    ref = B.bigvgan_forward(sd, B.BIGVGAN_V2_24K_100B_256X, mel)
    got = voc(mel)
    mx, rms = _report("bigvgan full t48", got, ref)
    clipped = (ref.abs() >= 1.0).float().mean().item()
    print(f"[parity] clipped fraction {clipped:.4f}")
    assert mx < 1e-4


# 1024: the shortest wave the host accepts (n_samples >= n_fft; 513 is below it); 256 x 94: an exact multiple of the hop;
# 256 x 94 + 255: one sample short of the next multiple
@pytest.mark.parametrize("b,nw", [(1, 120_000), (2, 24_000 + 77), (1, 1024), (2, 256 * 94), (1, 256 * 94 + 255)])
def test_mel_spectrogram_bigvgan(b, nw):
    from tts_indic_server_f5_amd.mel import mel_spectrogram_bigvgan
    wave = torch.cat([synth.ref_audio(nw, seed=1234 + i) for i in range(b)], dim=0)
    ref = _mel_float64(wave)
    got = mel_spectrogram_bigvgan(wave.cuda())
    assert got.shape == ref.shape == (b, 100, nw // 256)
    mx, rms = _report(f"bigvgan-mel b{b} nw{nw}", got, ref)
    assert rms < 1e-3 and mx < 5e-3


def _fp64(sd):
    return {k: v.double() for k, v in sd.items()}


# geometries the default checkpoint does not use: rate 8 and a final 32 channels; 128 mel channels (no padded mel channel) with a rate-8
# first stage and a final 4 channels; a final 48 channels, where the generator takes the naive conv_post (LDS tile above 48 KB)
GEOMS = {
    "r8822_c512": dict(upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), upsample_initial_channel=512),
    "mel128_r842222_c256": dict(num_mels=128, upsample_rates=(8, 4, 2, 2, 2, 2), upsample_kernel_sizes=(16, 8, 4, 4, 4, 4), upsample_initial_channel=256),
    "r222_c384": dict(upsample_rates=(2, 2, 2), upsample_kernel_sizes=(4, 4, 4), upsample_initial_channel=384),
}


@pytest.mark.parametrize("t", [128, 1])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_bigvgan_geometries_vs_fp64(geom, t):
    """Batch 3 at T = 128 (the first stage's pitch equals T: no padding row anywhere) and T = 1, against the float64 oracle, 1e-4 as the
    default geometry."""
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    arch = GEOMS[geom]
    sd = synth.bigvgan_state_dict(**arch)
    voc = F5HipBigVGAN(sd, **arch)
    g = torch.Generator().manual_seed(300 + t)
    mel = torch.randn(3, arch.get("num_mels", 100), t, generator=g) * 1.5 - 1.0
    ref = B.bigvgan_forward(_fp64(sd), B.BigVGANConfig(**arch), mel.double())
    got = voc(mel)
    up = 1
    for r in arch["upsample_rates"]:
        up *= r
    assert got.shape == ref.shape == (3, 1, up * t)
    mx, rms = _report(f"bigvgan {geom} b3 t{t} vs fp64", got, ref)
    assert mx < 1e-4


@pytest.mark.parametrize("b,t", [(2, 13), (1, 130)])
def test_bigvgan_wide_snake_spread(b, t):
    """The small config with the SnakeBeta log-parameters drawn from N(0, 0.6^2) instead of N(0, 0.2^2) (alpha and 1 / beta up to ~6 at
    3 sigma), against the float64 oracle at the default bound."""
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    sd = synth.bigvgan_state_dict(snake_scale=0.6, upsample_initial_channel=256)
    voc = F5HipBigVGAN(sd, upsample_initial_channel=256)
    g = torch.Generator().manual_seed(400 + t)
    mel = torch.randn(b, 100, t, generator=g) * 1.5 - 1.0
    cfg = B.BigVGANConfig(upsample_initial_channel=256)
    ref = B.bigvgan_forward(_fp64(sd), cfg, mel.double())
    _report(f"bigvgan wide snake spread b{b} t{t}: fp32 oracle", B.bigvgan_forward(sd, cfg, mel), ref)
    mx, rms = _report(f"bigvgan wide snake spread b{b} t{t}", voc(mel), ref)
    assert mx < 1e-4


def test_bigvgan_small_config_bf16_mode():
    """gemm_planes=1 (plain bf16 operands, bench.py --vocoder-planes 1).  Not a parity mode, like the fp16 mode whose test bounds 11-bit
    operands at 2.5e-3 max / 5e-4 rms: the operand rounding errors that dominate both scale with the unit roundoff, 2^-8 for bf16 against
    2^-11 for fp16, so the bound here is 8x that one: 2e-2 max, 4e-3 rms (against the float64 oracle)."""
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    sd = synth.bigvgan_state_dict(upsample_initial_channel=256)
    voc = F5HipBigVGAN(sd, upsample_initial_channel=256, gemm_planes=1)
    g = torch.Generator().manual_seed(213)
    mel = torch.randn(2, 100, 13, generator=g) * 1.5 - 1.0
    ref = B.bigvgan_forward(_fp64(sd), B.BigVGANConfig(upsample_initial_channel=256), mel.double())
    mx, rms = _report("bigvgan bf16 mode c0=256 b2 t13", voc(mel), ref)
    assert mx < 2e-2 and rms < 4e-3
