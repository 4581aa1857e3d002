"""CPU: the shaped-grain part of csrc/wave_formant_core.h as a stand-alone program (tools/wave_shape_check.cpp) built with the host C++
compiler under AddressSanitizer and UBSan.  The test passes the marks in; the program must print `wave_codec.psola_shape_pcm16`."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from tts_indic_server_f5_amd import wave_codec

from test_formant_host import LENGTHS, content
from test_shape_host import KINDS, MOVES


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/wave_formant_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("wave_shape_check") / "wave_shape_check"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                        os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "wave_shape_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("kind", KINDS)
def test_case_matrix_prints_the_host_samples(checker, tmp_path, kind):
    half, grains, drift, reach, stage, run = (int(v) for v in subprocess.run([checker, "--constants"], capture_output=True, text=True, check=True).stdout.split())
    assert half == max(400 * q // p for p, q in wave_codec.PITCH_RATIOS.values()) == 565 and grains == (2048 + 2 * half - 1) // 33 + 1 and run == 8
    assert drift > max(400 * abs(p - q) // p for p, q in wave_codec.PITCH_RATIOS.values()) + 1 and reach >= 400 + drift + 1 and reach % 8 == 0 and stage == 2048 + 2 * reach
    files, want = [], []
    for n in LENGTHS:
        x = content(kind, n)
        a, T, v = wave_codec.psola_marks(x, *wave_codec.psola_track(x))
        for s, f in MOVES:
            u, idx = wave_codec.psola_synthesis(a, T, v, n, s)
            P, Q = wave_codec.PITCH_RATIOS[f] if f else (1, 1)
            marks = np.stack([a, T, v], axis=1).astype("<i4").tobytes() + np.stack([u, idx], axis=1).astype("<i4").tobytes()
            files.append(tmp_path / f"case{len(files)}.bin")
            files[-1].write_bytes(struct.pack("<5i", P, Q, n, len(a), len(u)) + marks + x.astype("<i2").tobytes())
            want.append([n] + wave_codec.psola_shape_pcm16(x, s, f).tolist())
    r = subprocess.run([checker] + [str(p) for p in files], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert [[int(t) for t in line.split()] for line in r.stdout.splitlines()] == want


def test_a_bad_case_is_refused(checker, tmp_path):
    for head in ((47, 29, 0, 0, 0), (1, 1, -1, 0, 0), (41, 29, 100, 9, 0)):               # a ratio beyond 41 / 29; a negative length; too many marks
        (tmp_path / "bad.bin").write_bytes(struct.pack("<5i", *head))
        r = subprocess.run([checker, str(tmp_path / "bad.bin")], capture_output=True, text=True)
        assert r.returncode == 2 and "refused" in r.stderr
