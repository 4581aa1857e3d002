"""CPU: pins the per-stage float64 references of tests/vocos_ref.py and the sensitivity of the per-stage GPU test
(tests/test_gpu_vocos_stages.py).

Chain check: the unrounded stage functions chained reproduce oracle.vocos_oracle.vocos_decode in float64, for a batch and for items of
their own lengths (1e-12: float64 re-association; the waves have rms 0.02).

Sensitivity table: one deliberate slip at a time is put into one stage, with the mode's operand model standing in for the GPU, and must
leave the tolerance the GPU test applies to that stage -- by MARGIN, overall or on the worst row:
  backbone stages   rms(got - exact) <= FACTOR x rms(model - exact), overall and on the worst row (tests/test_gpu_blocks.py's rule);
  frames            per frame, rms(got - exact) / rms(exact) <= FRAME_FACTOR x the same figure of torch's fp32 irfft on the same input;
  overlap-add       per sample, |got - exact| <= OLA_ULPS 2^-24 sum|terms| / envelope.

What the rule cannot see (UNDETECTABLE, asserted as such): LayerNorm eps 1e-5 instead of 1e-6 -- the rows' variances are of order 1, so
the slip scales a row by 1 - 4.5e-6 / var: 0.4 .. 0.7 of the split-bf16 tolerance in every stage, and 5e-7 max on the wave with all ten
LayerNorms slipped at once (test_eps_slip_moves_the_wave_by_1e_7).
In the plain-bf16 mode (gemm_planes = 1) the model's own error is 2^-9 per operand, and tanh GELU (3e-4 on the hidden activations) and
the lo planes (there are none) are below it as well: BELOW_MODE1."""
import math

import pytest
import torch

import vocos_ref as R
from mel_ref import float64 as _float64
from oracle import vocos_oracle as V
from tts_indic_server_f5_amd import synth

FACTOR = 3.0         # backbone stages: gpu_err <= FACTOR x model_err (tests/test_gpu_vocos_stages.py)
FRAME_FACTOR = 4.0   # istft_frame_kernel: device expf / sinf / cosf at a few ulp against <= 1 on the CPU, and the table twiddles
OLA_ULPS = 10.0      # istft_ola_kernel: <= 4 terms and 4 squares of the fp32 window summed in fp32 (3 + 3 roundings, 2 per square), one division
MARGIN = 2.0         # a caught slip leaves the tolerance by at least this factor

# (slip, stage, the modes (gemm_planes) whose tolerance must catch it)
MUTATIONS = [
    ("tanh_gelu", "block", (2,)),
    ("pw1_a_lo_lost", "block", (2,)),
    ("pw1_w_lo_lost", "block", (2,)),
    ("pw2_a_lo_lost", "block", (2,)),
    ("pw2_w_lo_lost", "block", (2,)),
    ("no_dwconv_bias", "block", (2, 1)),
    ("no_pwconv2_bias", "block", (2, 1)),
    ("no_gamma", "block", (2, 1)),
    ("replicate_padding", "block", (2, 1)),
    ("reads_neighbours", "block", (2, 1)),
    ("replicate_padding", "embed", (2, 1)),
    ("symmetric_hann", "frames", (2, 1)),
    ("nyquist_imag_kept", "frames", (2, 1)),
    ("no_clip", "frames", (2, 1)),
    ("envelope_without_squares", "ola", (2, 1)),
]
UNDETECTABLE = [("eps_1e-5", "embed"), ("eps_1e-5", "block"), ("eps_1e-5", "head")]
BELOW_MODE1 = [("tanh_gelu", "block")]


def _mel(t, seed):
    return torch.randn(100, t, generator=torch.Generator().manual_seed(seed)) * 1.5 - 1.0


@pytest.fixture(scope="module")
def weights():
    return R.Weights(synth.vocos_state_dict())


# ---------------------------------------------------------------------------------------------------------------- chain check
def _oracle(W, mel):
    return _float64(V.vocos_decode, W.sd, mel.double())


def test_chain_reproduces_vocos_decode_batched(weights):
    g = torch.Generator().manual_seed(7)
    mel = torch.randn(3, 100, 21, generator=g) * 1.5 - 1.0
    ref = _oracle(weights, mel)
    assert ref.dtype == torch.float64 and ref.shape == (3, 256 * 20)
    for i in range(3):
        assert (R.decode(weights, mel[i]) - ref[i]).abs().max().item() < 1e-12


@pytest.mark.parametrize("t", [2, 3, 7, 130])
def test_chain_reproduces_vocos_decode_item_lengths(weights, t):
    """Items shorter than the 7-tap kernels, exactly as long, and longer than a 128-row slab; every stage's shape on the way"""
    mel = _mel(t, 40 + t)
    xs = R.backbone(weights, mel)
    y = R.head(weights, xs[-1])
    fw = R.frames(y)
    assert len(xs) == 9 and all(x.shape == (t, 512) for x in xs) and y.shape == (t, 1026) and fw.shape == (t, 1024)
    wave = R.ola(fw)
    assert wave.shape == (256 * (t - 1),)
    assert (wave - _oracle(weights, mel[None])[0]).abs().max().item() < 1e-12
    assert torch.equal(wave, R.decode(weights, mel))


def test_mode_models_are_what_the_issue_measured(weights):
    """The split-bf16 model of the whole decode is ~5e-7 max / ~1e-7 rms off float64 (the library measures 7.5e-7 on an MI355X), the
    plain-bf16 one three orders above: the two tolerances of the tightened whole-decode tests."""
    mel = _mel(77, 177)
    exact = R.decode(weights, mel)
    err = {p: R.decode(weights, mel, R.MODES[p]) - exact for p in (2, 1)}
    for p, e in err.items():
        print(f"[model] gemm_planes {p}: whole decode max {e.abs().max():.3e} rms {e.pow(2).mean().sqrt():.3e} (wave rms {exact.pow(2).mean().sqrt():.3f})")
    assert 1e-7 < err[2].abs().max().item() < 2e-6
    assert 100 * err[2].abs().max().item() < err[1].abs().max().item() < 1e-2


# ---------------------------------------------------------------------------------------------------------------- sensitivity table
def _ratio(got, exact, model):
    """how far `got` is outside FACTOR x the model's error: the smaller of (overall, worst row) must exceed 1 to pass, so a slip is caught
    when the larger exceeds 1"""
    g, m = R.row_stats(got - exact), R.row_stats(model - exact)
    return max(g[0] / (FACTOR * m[0]), g[1] / (FACTOR * m[1]))


def frame_rel(got, exact):
    """per frame: rms(got - exact) / rms(exact)"""
    return ((got.double() - exact).pow(2).mean(dim=-1) / exact.pow(2).mean(dim=-1)).sqrt()


def ola_bound(fw):
    """per sample: OLA_ULPS 2^-24 sum|terms| / envelope"""
    _, mag, env = R.ola_terms(fw)
    return OLA_ULPS * 2.0 ** -24 * mag / env


@pytest.fixture(scope="module")
def sites(weights):
    """per stage: fn(mode, mut) -> how many times the slip's output (the mode's model with the slip) is outside that stage's tolerance"""
    W = weights
    mels = [_mel(t, 60 + t) for t in (9, 20, 6)]                 # the middle item is the one looked at; the others are its neighbours
    x3 = [R.backbone(W, m, num_layers=3)[-1] for m in mels]      # block 3: its input has been through three blocks
    before, after = x3[0][-3:], x3[2][:3]
    x8 = R.backbone(W, mels[1])[-1]
    out = {}

    def stage(name, fn):
        exact = fn(R.EXACT, ())
        model = {p: fn(R.MODES[p], ()) for p in (2, 1)}
        out[name] = lambda p, mut: _ratio(fn(R.MODES[p], (mut,)), exact, model[p])

    stage("embed", lambda F, mut: R.embed(W, mels[1], F, mut))
    stage("block", lambda F, mut: R.block(W, 3, x3[1], F, mut, before, after))
    stage("head", lambda F, mut: R.head(W, x8, F, mut))

    # frames: the state of test_vocos_decode_magnitude_clip (log-magnitudes raised by ln 100, half the bins clipped)
    sd = dict(W.sd)
    sd["head.out.bias"] = sd["head.out.bias"].clone()
    sd["head.out.bias"][:513] += math.log(100.0)
    y = R.head(R.Weights(sd), x8).float()
    assert 0.2 < (y[:, :513] > math.log(100.0)).double().mean().item() < 0.8
    fw = R.frames(y)
    tol_frames = FRAME_FACTOR * frame_rel(R.frames(y, dtype=torch.float32), fw)
    out["frames"] = lambda p, mut: (frame_rel(R.frames(y, (mut,), torch.float32), fw) / tol_frames).max().item()
    tol_ola = ola_bound(fw.float())
    wave = R.ola(fw.float())
    out["ola"] = lambda p, mut: ((R.ola(fw.float(), (mut,)).float().double() - wave).abs() / tol_ola).max().item()
    out["_unmutated"] = {"frames": (frame_rel(R.frames(y, dtype=torch.float32), fw) / tol_frames).max().item(),
                         "ola": ((wave.float().double() - wave).abs() / tol_ola).max().item()}
    return out


def test_unmutated_stand_ins_pass(sites):
    """The fp32 computations that stand in for the GPU in the frames and overlap-add rows pass their own rules"""
    print(f"[sensitivity] unmutated: frames {sites['_unmutated']['frames']:.3f}, ola {sites['_unmutated']['ola']:.3f} x the tolerance")
    assert sites["_unmutated"]["frames"] == 1.0 / FRAME_FACTOR and sites["_unmutated"]["ola"] < 0.2


def test_sensitivity_table(sites):
    """Every slip a mode claims leaves that stage's tolerance by at least MARGIN; eps 1e-5 stays inside it in every stage, and so does
    tanh GELU in the plain-bf16 mode."""
    bad = []
    for name, where, modes in MUTATIONS + [(n, w, ()) for n, w in UNDETECTABLE]:
        ratio = {p: sites[where](p, name) for p in (2, 1)}
        print(f"[sensitivity] {name:26s} in {where:7s}: {ratio[2]:12.2f} x the tolerance of gemm_planes 2, {ratio[1]:10.2f} x that of 1")
        for p in (2, 1):
            if p in modes and ratio[p] < MARGIN:
                bad.append((name, where, p, ratio[p]))
            if p == 1 and (name, where) in BELOW_MODE1 and ratio[1] >= 1.0:
                bad.append((name, where, "no longer below the plain-bf16 floor", ratio[1]))
        if not modes and max(ratio.values()) >= 1.0:
            bad.append((name, where, "listed as undetectable", ratio))
    assert not bad, bad


def test_eps_slip_moves_the_wave_by_1e_7(weights):
    """What UNDETECTABLE costs: eps 1e-5 in all ten LayerNorms at once moves the wave by 5.2e-7 max, 1e-7 rms -- the size of the
    split-bf16 model's own distance from float64 (4.6e-7 max) and inside the 3 x of the whole-decode tests, so no test of this suite
    can see it and none pretends to."""
    mel = _mel(77, 177)
    exact = R.decode(weights, mel)
    d = R.decode(weights, mel, mut=("eps_1e-5",)) - exact
    m = R.decode(weights, mel, R.MODES[2]) - exact
    print(f"[sensitivity] eps 1e-5 in every LayerNorm: wave max {d.abs().max():.3e} rms {d.pow(2).mean().sqrt():.3e}; "
          f"split-bf16 model max {m.abs().max():.3e} rms {m.pow(2).mean().sqrt():.3e}")
    assert d.abs().max().item() < FACTOR * m.abs().max().item() and d.pow(2).mean().sqrt().item() < FACTOR * m.pow(2).mean().sqrt().item()
    assert d.abs().max().item() < 1e-6
