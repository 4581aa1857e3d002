"""GPU: the ragged BigVGAN forward (`F5HipBigVGAN.decode_ragged`, f5hip_bigvgan_forward_ragged, torch.ops.f5hip.bigvgan_forward_ragged): every
item of one call against the same item vocoded alone (to the last bit) and against the float64 oracle, on the reduced-width generator that
tests/test_gpu_bigvgan.py builds (initial channel 256, seeded random weights).

No end-to-end test through `infer_requests` / `infer_process_stream` here: tests/conftest.py offers no tiny model fixture to run one with; the
host side of that path (`infer._chunk_waves`) is covered by tests/test_bigvgan_ragged_host.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import bigvgan_oracle as B  # noqa: E402
from tts_indic_server_f5_amd import _lib, synth  # noqa: E402

C0 = 256
UP = 256
# an item's end on, just before and just after the 128-row pitch of the first stage; one frame (every tap reads padding); two short ones
FRAMES = [1, 5, 127, 128, 129, 37]
MODES = [2, 3, 1]   # gemm_planes: split bf16, fp16, bf16


@pytest.fixture(scope="module")
def sd():
    return synth.bigvgan_state_dict(upsample_initial_channel=C0)


def _make(sd, planes=2):
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    return F5HipBigVGAN(sd, upsample_initial_channel=C0, gemm_planes=planes)


@pytest.fixture(scope="module")
def vocs(sd):
    return {p: _make(sd, p) for p in MODES}


@pytest.fixture(scope="module")
def mels():
    g = torch.Generator().manual_seed(511)
    return [torch.randn(100, t, generator=g) * 1.5 - 1.0 for t in FRAMES]


@pytest.fixture(scope="module")
def alone(vocs, mels):
    """Every item vocoded by a call of its own, per mode: computed once, never modified."""
    return {p: [v(m[None]).reshape(-1).clone() for m in mels] for p, v in vocs.items()}


def _same(a, b, tag):
    assert a.shape == b.shape, f"{tag}: {tuple(a.shape)} vs {tuple(b.shape)}"
    assert torch.equal(a, b), f"{tag}: max diff {(a - b).abs().max().item():.3e}"


@pytest.mark.parametrize("planes", MODES)
def test_each_item_equals_its_own_call(vocs, mels, alone, planes):
    got = vocs[planes].decode_ragged(mels)
    assert [w.shape for w in got] == [(UP * t,) for t in FRAMES]
    for t, a, w in zip(FRAMES, alone[planes], got):
        _same(w, a, f"planes {planes} T={t}")


def test_items_vs_fp64_oracle(vocs, mels, sd):
    """The bound of tests/test_gpu_bigvgan.py for the uniform forward in the parity mode: 1e-4 max on waveform samples."""
    got = vocs[2].decode_ragged(mels)
    sd64 = {k: v.double() for k, v in sd.items()}
    for t, m, w in zip(FRAMES, mels, got):
        ref = B.bigvgan_forward(sd64, B.BigVGANConfig(upsample_initial_channel=C0), m[None].double()).reshape(-1)
        mx = (w.cpu().double() - ref).abs().max().item()
        print(f"[parity] bigvgan ragged T={t} vs fp64: max_err {mx:.3e}")
        assert mx < 1e-4


def _packed_call(voc, slab, frames):
    """The C entry point through ctypes on a caller-made slab [n][100][T_max]"""
    f = torch.tensor(frames, dtype=torch.int32)
    slab = slab.cuda().contiguous()
    wave = torch.empty(UP * sum(frames), device="cuda")
    _lib.check(_lib.lib().f5hip_bigvgan_forward_ragged(voc._h, len(frames), C.c_void_p(f.data_ptr()), C.c_void_p(slab.data_ptr()),
                                                       C.c_void_p(wave.data_ptr()), _lib.current_stream_ptr()), "bigvgan_forward_ragged")
    return wave


def _slab(mels, fill):
    slab = torch.full((len(mels), 100, max(m.shape[1] for m in mels)), fill)
    for i, m in enumerate(mels):
        slab[i, :, :m.shape[1]] = m
    return slab


@pytest.mark.parametrize("fill", [1e30, float("nan")])
def test_padding_columns_are_not_read(vocs, mels, fill):
    zero = _packed_call(vocs[2], _slab(mels, 0.0), FRAMES)
    _same(_packed_call(vocs[2], _slab(mels, fill), FRAMES), zero, f"padding {fill}")


def test_order_and_company_do_not_matter(vocs, mels, alone):
    order = [4, 0, 3, 5, 1, 2]
    got = vocs[2].decode_ragged([mels[i] for i in order])
    for i, w in zip(order, got):
        _same(w, alone[2][i], f"permuted T={FRAMES[i]}")
    # a short item between two long ones, against the same item alone in a ragged call
    for i in (0, 5):
        mid = vocs[2].decode_ragged([mels[4], mels[i], mels[3]])[1]
        _same(mid, vocs[2].decode_ragged([mels[i]])[0], f"between long items T={FRAMES[i]}")
        _same(mid, alone[2][i], f"between long items vs own call T={FRAMES[i]}")


def test_workspace_reuse(sd, vocs, mels):
    """long ragged call, short ragged call, uniform batch of 2 on ONE object: each equals its result on a fresh object (no row a larger
    earlier call left behind is read)"""
    long_items, short_items = [mels[4], mels[3], mels[2]], [mels[1], mels[0], mels[5]]
    g = torch.Generator().manual_seed(77)
    uni = torch.randn(2, 100, 13, generator=g) * 1.5 - 1.0
    v = _make(sd)
    seq = [v.decode_ragged(long_items), v.decode_ragged(short_items), [v(uni).reshape(-1)]]
    fresh = [_make(sd).decode_ragged(long_items), _make(sd).decode_ragged(short_items), [_make(sd)(uni).reshape(-1)]]
    for k, (a, b) in enumerate(zip(seq, fresh)):
        for j, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"call {k} item {j}")


def test_ctypes_and_torch_op_paths_agree(vocs, mels, alone):
    from tts_indic_server_f5_amd import torch_ops
    packed = _packed_call(vocs[2], _slab(mels, 0.0), FRAMES)
    _same(packed, torch.cat(alone[2]), "ctypes")
    assert torch_ops.load(), "the torch operator library must be built"
    op = torch_ops.ops().bigvgan_forward_ragged(int(vocs[2]._h), _slab(mels, 0.0).cuda(), torch.tensor(FRAMES, dtype=torch.int32), 100, UP)
    _same(op, packed, "torch op vs ctypes")
    _same(torch.cat(vocs[2].decode_ragged(mels)), packed, "decode_ragged vs ctypes")


def test_argument_errors(vocs, mels, alone):
    v = vocs[2]
    assert v.decode_ragged([]) == []
    for bad in ([mels[1], torch.zeros(100, 0)], [mels[1], torch.zeros(80, 5)], [mels[1], torch.zeros(1, 100, 5)]):
        with pytest.raises(_lib.F5HipError):
            v.decode_ragged(bad)
    f = torch.tensor([5, 0], dtype=torch.int32)
    x = torch.zeros(2, 100, 5, device="cuda")
    w = torch.zeros(UP * 5, device="cuda")
    lib = _lib.lib()
    assert lib.f5hip_bigvgan_forward_ragged(v._h, 2, C.c_void_p(f.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), None) != 0
    assert lib.f5hip_bigvgan_forward_ragged(v._h, 0, C.c_void_p(f.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), None) != 0
    assert lib.f5hip_bigvgan_forward_ragged(v._h, 2, None, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), None) != 0
    for t, a, got in zip(FRAMES, alone[2], v.decode_ragged(mels)):
        _same(got, a, f"after the errors T={t}")


# ---------------------------------------------------------------------------------------------------------------- the default geometry
FULL_FRAMES = [300, 1, 257, 256, 130]   # pitches 384 / 128 / 384 / 256 / 256: both first-stage paths, items over more than two first-stage blocks


@pytest.mark.parametrize("planes", [2, 3])
def test_default_geometry_items_equal_their_own_calls(planes):
    """bigvgan_v2_24khz_100band_256x at full width (stage widths 768 ... 24: the wide conv5 tiles, several column tiles, the XCD-blocked tile
    order): every item of one ragged call equals its own uniform call to the last bit, in the caller's order and permuted.  No oracle here:
    tests/test_gpu_bigvgan.py pins the uniform call at this geometry."""
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN
    voc = F5HipBigVGAN(synth.bigvgan_state_dict(), gemm_planes=planes)
    g = torch.Generator().manual_seed(523)
    mels = [torch.randn(100, t, generator=g) * 1.5 - 1.0 for t in FULL_FRAMES]
    own = [voc(m[None]).reshape(-1).clone() for m in mels]
    for order in (list(range(len(mels))), [3, 1, 0, 4, 2]):
        got = voc.decode_ragged([mels[i] for i in order])
        for i, w in zip(order, got):
            assert w.shape == (UP * FULL_FRAMES[i],)
            _same(w, own[i], f"full width planes {planes} order {order} T={FULL_FRAMES[i]}")
        print(f"[parity] bigvgan ragged full width planes {planes} order {order}: {len(order)} items bit-equal to their own calls (bound 0)")
