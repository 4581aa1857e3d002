"""CPU: the linear-domain mel bound of tests/mel_ref.py is reachable and tight.  The fp32 oracle, run against the float64 oracle, stays inside
it on every signal and for both front-ends (this is what fixes the constants r and a, by the recipe written beside them); and each of seven
subtly wrong float64 front-ends, built here from the oracle's own pieces, falls outside it on a named signal.  The GPU tests of
tests/test_gpu_mel_levels.py hold mel_frame_kernel to the same bound."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import mel_ref as M
from oracle import bigvgan_oracle as B
from oracle import vocos_oracle as V


@functools.lru_cache(maxsize=None)
def _refs(front):
    """name -> (wave, float64 log-mel, fp32-oracle log-mel) at the default geometry."""
    return {k: (w, M.ref64(front, w), M.oracle32(front, w)) for k, w in M.signals_for(front).items()}


def test_signals_are_deterministic_and_cover_the_regimes():
    s, s2 = M.signals(), M.signals()
    assert all(torch.equal(s[k], s2[k]) for k in s)
    assert all(w.dtype == torch.float32 and w.ndim == 2 and w.shape[1] <= M.NW for w in s.values())
    assert s["tones_513"].shape[1] == 513 and s["tones_1024"].shape[1] == 1024
    assert s["clipped"].abs().max().item() == 1.0 and (s["clipped"].abs() == 1.0).float().mean().item() > 0.2
    for front in M.FRONTS:
        r = _refs(front)
        z = {k: int(M.zero_frames(front, w).sum()) for k, (w, _, _) in r.items()}
        t = r["zeros"][1].shape[-1]
        assert z["zeros"] == t and 0 < z["tones_then_zeros"] < t // 2 and 0 < z["impulse"] < t
        assert t - z["impulse"] in (4, 5)                                        # the frames that hold the impulse
        assert z["control"] == z["tones"] == z["edge_steps"] == 0
        # partly silent frames at the boundary: some frame is neither all-zero nor untouched by the zeros
        w = r["tones_then_zeros"][0]
        pad = M.PAD_HOP[front](1024, 256)
        frames = F.pad(w.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1).unfold(-1, 1024, 256)
        partly = ((frames == 0).float().mean(-1) > 0.05) & ~(frames == 0).all(-1)
        assert partly.sum().item() >= 3
        # where the log-domain bounds of the older tests apply (decided from the float64 reference)
        for k in ("dc_tones_noise", "clipped"):
            assert M.far_above_floor(r[k][1]), (front, k)
        for k in ("tones", "loud_low_tone", "dc_plus_tones", "zeros", "impulse"):
            assert not M.far_above_floor(r[k][1]), (front, k)
            assert (r[k][1] == M.LOG_CLAMP).any(), (front, k)                    # bins at the clamp itself


@pytest.mark.parametrize("front", M.FRONTS)
def test_constants_follow_the_recipe(front):
    """r = 4 max |E32 - E64| / E64 on the control signal, a = 4 max (|E32 - E64| - r E64) / P_t on the others: the constants in mel_ref are
    these, rounded up.  Another FFT library rounds differently, so what is asserted is that they lie between 0.9 and 2 times the recipe on
    the machine that runs this; that the fp32 oracle is inside the bound is the next test."""
    r, a = M.BOUND[front]
    refs = _refs(front)
    _, r64, r32 = refs[M.CONTROL]
    r_meas = ((r32.double().exp() - r64.exp()).abs() / r64.exp()).max().item()
    a_meas = 0.0
    for k, (_, r64, r32) in refs.items():
        if k != M.CONTROL:
            a_meas = max(a_meas, M.linear_parts(r32, r64, r, 0.0)[1])
    print(f"[parity] {front} fp32 oracle vs float64: r measured {r_meas:.3e} (x4 = {4 * r_meas:.3e}, r = {r:.2e}), "
          f"a measured {a_meas:.3e} (x4 = {4 * a_meas:.3e}, a = {a:.2e})")
    assert 0.9 * 4 * r_meas <= r <= 2 * 4 * r_meas
    assert 0.9 * 4 * a_meas <= a <= 2 * 4 * a_meas


@pytest.mark.parametrize("front", M.FRONTS)
def test_fp32_oracle_is_inside_the_bound_on_every_signal(front):
    r, a = M.BOUND[front]
    for k, (w, r64, r32) in _refs(front).items():
        M.check_linear(r32, r64, r, a, tag=f"{front} fp32 oracle, {k}")
        M.check_exact_frames(r32, M.zero_frames(front, w), tag=f"{front} fp32 oracle, {k}")
        M.check_exact_frames(r64, M.zero_frames(front, w), tag=f"{front} float64 oracle, {k}")


def test_bigvgan_magnitude_floor_stays_under_the_clamp():
    """On an all-zero frame the BigVGAN front-end's magnitudes are sqrt(1e-9) and a channel is sqrt(1e-9) times its Slaney filter's sum.
    In float64 that stays under the clamp of 1e-5 for the default geometry and every geometry of M.GEOMETRIES, so such frames give
    log(1e-5) exactly."""
    for name, g in {"default": {}, **M.GEOMETRIES}.items():
        g = M._geom(**g)
        fb = B.librosa_slaney_mel(g["sr"], g["n_fft"], g["n_mels"]).double()
        worst = (fb.sum(-1) * math.sqrt(1e-9)).max().item()
        print(f"[parity] bigvgan zero-frame channel before the clamp, {name}: {worst:.3e}")
        assert worst < 0.5 * M.CLAMP
    z = M.ref64("bigvgan", torch.zeros(1, 4096))
    assert torch.equal(z, torch.full_like(z, M.LOG_CLAMP))


# ------------------------------------------------------------------------------------------------ perturbed float64 front-ends
def _htk_fbanks(n_freqs, f_nyquist, f_max, n_mels):
    """V.melscale_fbanks_htk with the bin frequencies (0 .. f_nyquist) kept apart from the filters' upper corner f_max, as torchaudio has
    them; the oracle passes one number for both."""
    all_freqs = torch.linspace(0, f_nyquist, n_freqs)
    m_pts = torch.linspace(V.hz_to_mel_htk(0.0), V.hz_to_mel_htk(f_max), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    return torch.clamp(torch.min((-1.0 * slopes[:, :-2]) / f_diff[:-1], slopes[:, 2:] / f_diff[1:]), min=0.0)


def _pieces(front, wave, periodic=True, pad_kind="reflect", fmax_scale=1.0, power=1, clamp=1e-5, eps=1e-9,
            n_fft=1024, hop=256, n_mels=100, sr=24000):
    """Either front-end in float64 from its pieces (explicit padding, Hann window, STFT without centring, magnitude, filterbank, clamp,
    log), each of which can be made subtly wrong."""
    def run():
        w = wave.double()
        pad = M.PAD_HOP[front](n_fft, hop)
        if pad_kind == "symmetric":                                              # x[-k] = x[k - 1]: reflection that repeats the end sample
            w = torch.cat([w[..., :pad].flip(-1), w, w[..., w.shape[-1] - pad:].flip(-1)], -1)
        else:
            w = F.pad(w.unsqueeze(1), (pad, pad), mode=pad_kind).squeeze(1)
        spec = torch.stft(w, n_fft, hop, n_fft, torch.hann_window(n_fft, periodic=periodic), center=False, return_complex=True)
        mag = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + (eps if front == "bigvgan" else 0.0))
        if power == 2:
            mag = mag * mag
        if front == "vocos":
            fb = _htk_fbanks(n_fft // 2 + 1, float(sr // 2), float(sr // 2) * fmax_scale, n_mels).T
        else:
            fb = B.librosa_slaney_mel(sr, n_fft, n_mels, fmax=sr / 2.0 * fmax_scale).double()
        return torch.matmul(fb, mag).clamp(min=clamp).log()
    return M.float64(run)


@pytest.mark.parametrize("front", M.FRONTS)
def test_unperturbed_pieces_are_the_oracle(front):
    for k, (w, r64, _) in _refs(front).items():
        assert (_pieces(front, w) - r64).abs().max().item() < 1e-11, (front, k)
    assert torch.equal(M.float64(_htk_fbanks, 513, 12000.0, 12000.0, 100), M.float64(V.melscale_fbanks_htk, 513, 0.0, 12000.0, 100))


# perturbation -> (what is wrong, the signal on which the bound must catch it)
PERTURBED = {
    "symmetric_hann": (dict(periodic=False), "control"),
    "reflect_off_by_one": (dict(pad_kind="symmetric"), "edge_steps"),
    "edge_replication": (dict(pad_kind="replicate"), "edge_steps"),
    "f_max_minus_0.1_percent": (dict(fmax_scale=0.999), "tones"),
    "power_spectrum": (dict(power=2), "loud_low_tone"),
    "clamp_1e-6": (dict(clamp=1e-6), "zeros"),
    "no_1e-9_under_the_root": (dict(eps=0.0), "faint_noise"),
}


# the Vocos front-end has no 1e-9 term to drop
@pytest.mark.parametrize("front,what", [(f, p) for f in M.FRONTS for p in PERTURBED if (f, p) != ("vocos", "no_1e-9_under_the_root")])
def test_perturbed_front_end_falls_outside_the_bound(front, what):
    kw, name = PERTURBED[what]
    r, a = M.BOUND[front]
    w, r64, _ = _refs(front)[name]
    got = _pieces(front, w, **kw)
    with pytest.raises(AssertionError, match="outside r E"):
        M.check_linear(got, r64, r, a, tag=f"{front} {what}, {name}")
    # and not by a hair: at least 10x the bound somewhere
    assert M.linear_parts(got, r64, r, a)[2].max().item() > 10.0


def test_check_linear_counts_every_bin():
    """One bin of 9 400 moved by twice its allowance fails; the same bins at 0.9 of it pass."""
    front = "vocos"
    r, a = M.BOUND[front]
    _, r64, _ = _refs(front)["tones"]
    e = r64.exp()
    allow = r * e + a * e.amax(-2, keepdim=True)
    M.check_linear((e + 0.9 * allow).log(), r64, r, a)
    M.check_linear((e - 0.9 * allow).clamp(min=1e-300).log(), r64, r, a)
    bad = e.clone()
    bad[0, 57, 31] += 2.0 * allow[0, 57, 31]
    with pytest.raises(AssertionError, match=r"1 of 9400 bins outside .* \[0, 57, 31\]"):
        M.check_linear(bad.log(), r64, r, a)
