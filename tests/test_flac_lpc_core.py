"""CPU: the level-1 FLAC encoder's shared core (csrc/flac_lpc_core.h: window, autocorrelation, Levinson-Durbin in fp64, quantisation and
the residual guard, the text wave_flac_frame_kernel<true> compiles) as a stand-alone program (tools/flac_lpc_check.cpp) built with the host
C++ compiler, contraction off, under AddressSanitizer and UBSan.  Its output is compared line for line with the Python definition in
`wave_codec` (and with the second Python writing of the rule in flac_lpc_ref.py): the validity, shift and coefficients of every order and
the guard's verdict.  This is where the fp64 exactness and the int32 bound of the residual sum are shown without a GPU.  No Python extension
and no preloaded library is involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import flac_lpc_ref as R
from tts_indic_server_f5_amd import wave_codec as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: csrc/flac_lpc_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("flac_lpc_check") / "flac_lpc_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "flac_lpc_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(checker, mode, path):
    r = subprocess.run([checker, mode, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def _definition_lines(blocks):
    """What the program must print for int16 blocks [F, 4096], from the host definition."""
    x = blocks.astype(np.int64)
    lines = []
    for f, Rf in enumerate(W.flac_lpc_autocorrelation(x)):
        coefs = W.flac_lpc_coefficients(Rf)
        for o in W.FLAC_LPC_ORDERS:
            if o not in coefs:
                lines.append(" ".join(str(v) for v in [o, 0, 0, 0] + [0] * o))
                continue
            q, shift = coefs[o]
            _, inside = W.flac_lpc_residual(x[f:f + 1], np.array([q], dtype=np.int64), np.array([shift]))
            lines.append(" ".join(str(v) for v in [o, 1, shift, int(inside[0])] + list(q)))
    return lines


def _matrix_blocks():
    sig = R.signals()
    return np.stack([x[at:at + R.BLOCK] for x in sig.values() for at in (0, R.BLOCK)])


def test_signal_matrix_line_for_line(checker, tmp_path):
    blocks = _matrix_blocks()
    path = tmp_path / "matrix.bin"
    blocks.astype("<i2").tofile(path)
    got = _run(checker, "blocks", path)
    assert got == _definition_lines(blocks)
    # the second writing of the rule, in Python ints and floats, on the first block of each signal
    for i in range(0, len(blocks), 2):
        for c, (o, (valid, shift, q, inside)) in enumerate(R.lpc_orders(blocks[i]).items()):
            assert got[4 * i + c] == " ".join(str(v) for v in [o, int(valid), shift, int(bool(inside))] + q)
    assert any(line.split()[1] == "1" for line in got) and any(line.split()[1] == "0" for line in got)


def test_two_hundred_filtered_noise_blocks(checker, tmp_path):
    blocks = R.filtered_noise_blocks(200)
    path = tmp_path / "random.bin"
    blocks.astype("<i2").tofile(path)
    got = _run(checker, "blocks", path)
    assert len(got) == 800 and got == _definition_lines(blocks)
    assert sum(line.split()[1] == "1" for line in got) >= 700          # the corpus exercises the recursion, not its exits


def test_guard_drops_a_hand_made_order(checker, tmp_path):
    """No block was found that reaches the guard through Levinson, so it is fed directly: q = [2047] * 12 at shift 0 on a loud block predicts
    far outside 16 bits; the same coefficients at shift 15 do not."""
    rng = np.random.default_rng(5)
    loud = np.where(rng.random(R.BLOCK) < 0.5, 32767, -32768).astype(np.int16)
    loud[:64] = 32767                                                   # twelve equal full-scale neighbours: the sum reaches 12 * 2047 * 32767
    q = np.full((1, 12), 2047, dtype=np.int64)
    path = tmp_path / "guard.bin"
    with open(path, "wb") as f:
        for shift in (0, 15):
            f.write(loud.astype("<i2").tobytes() + np.array([2047] * 12 + [shift], dtype="<i4").tobytes())
    got = _run(checker, "guard", path)
    want = [str(int(W.flac_lpc_residual(loud.astype(np.int64)[None], q, np.array([shift]))[1][0])) for shift in (0, 15)]
    assert got == want == ["0", "1"]
    assert [int(R.residual_inside(loud, [2047] * 12, s)) for s in (0, 15)] == [0, 1]
