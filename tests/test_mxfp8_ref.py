"""tests/mxfp8_ref.py, the numpy restatement of the MXFP8 definition in csrc/gemm8.h, on hand-picked blocks."""
import numpy as np
import pytest

from mxfp8_ref import dequant, e4m3_decode, e4m3_encode, quant


def _block(**at):
    b = np.zeros(32)
    for i, v in at.items():
        b[int(i[1:])] = v
    return b


# (block, exponent, {index: expected dequantised value})
CASES = {
    "zeros": (_block(), -127, {0: 0.0, 31: 0.0}),
    "lone_448": (_block(k5=448.0), 0, {5: 448.0}),                           # floor(log2 448) = 8
    "amax_power_of_two": (_block(k0=-4.0, k1=1.0), -6, {0: -4.0, 1: 1.0}),   # 4 = 2^2 -> e = -6, element 256
    "rounds_into_next_binade": (_block(k0=256.0, k1=31.5), 0, {1: 32.0}),    # 31.5 between 30 and 32 (step 2): the tie goes to the even mantissa, 32
    "tie_to_even": (_block(k0=256.0, k1=17.0, k2=19.0), 0, {1: 16.0, 2: 20.0}),   # step 2 in [16, 32): 17 -> 16 (mantissa 0), 19 -> 20 (mantissa 2)
    "subnormal_result": (_block(k0=256.0, k1=2.0 ** -9 * 3, k2=2.0 ** -11, k3=2.0 ** -10), 0, {1: 2.0 ** -9 * 3, 2: 0.0, 3: 0.0}),   # 2^-10: tie to 0
    "saturates": (_block(k0=500.0, k1=-460.0), 0, {0: 448.0, 1: -448.0}),    # e = 0; 460 and 500 lie beyond the largest E4M3
    "clamp_low": (_block(k0=2.0 ** -140, k1=-2.0 ** -141), -127, {0: 0.0, 1: -0.0}),   # floor(log2) - 8 = -148 -> -127; elements 2^-13, -2^-14 -> +-0
    "clamp_high": (_block(k0=2.0 ** 200), 127, {0: 448.0 * 2.0 ** 127}),     # e would be 192: clamped, the element saturates
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_picked_blocks(name):
    block, e_want, values = CASES[name]
    codes, e = quant(block[None])
    assert e.shape == (1, 1) and int(e[0, 0]) == e_want
    back = dequant(codes, e)[0]
    for i, v in values.items():
        assert back[i] == v and np.signbit(back[i]) == np.signbit(v), (i, back[i], v)


def test_nonfinite_poisons_its_block_only():
    x = np.ones((2, 64))
    x[0, 40], x[1, 3] = np.inf, np.nan
    back = dequant(*quant(x))
    assert np.isnan(back[0, 32:]).all() and np.isnan(back[1, :32]).all()
    assert (back[0, :32] == 1.0).all() and (back[1, 32:] == 1.0).all()


def test_element_rounding_matches_torch_float8():
    torch = pytest.importorskip("torch")
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("this torch has no float8_e4m3fn")
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-448, 448, 4096), rng.uniform(-1, 1, 4096) * 2.0 ** rng.integers(-12, 0, 4096),
                        np.arange(0, 1024) * 2.0 ** -10, [448.0, -448.0, 0.0]]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    assert np.array_equal(e4m3_decode(e4m3_encode(x)), want)
