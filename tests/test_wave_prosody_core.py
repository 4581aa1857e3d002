"""CPU: the WSOLA launch's core (csrc/wave_prosody_core.h: the index geometry, the tie rule and the blend the kernel compiles) as a
stand-alone program (tools/wave_prosody_check.cpp) built with the host C++ compiler under AddressSanitizer and UBSan.  It runs the kernel's
frame loop serially -- window and target staging, the search over the packed key, the blend from the staged copies -- with the samples, the
window, the target and the output each in a heap block of exactly its size, so a read or write out of bounds is a report and a non-zero
exit.  It must print the frame starts and the samples of `wave_codec._wsola_frames`.  No Python extension and no preloaded library is
involved."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tts_indic_server_f5_amd import wave_codec

from test_prosody_host import CONTENTS, LENGTHS, STRETCHES, _content

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/wave_prosody_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("wave_prosody_check") / "wave_prosody_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "wave_prosody_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(checker, tmp_path, items):
    """[(frame starts, samples)] of the program over (x, P, Q) items; it must exit 0 with nothing from a sanitizer."""
    files = []
    for i, (x, P, Q) in enumerate(items):
        p = tmp_path / f"case{i}.bin"
        p.write_bytes(struct.pack("<3i", P, Q, len(x)) + x.astype("<i2").tobytes())
        files.append(str(p))
    r = subprocess.run([checker] + files, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = [[int(t) for t in line.split()] for line in r.stdout.splitlines()]
    assert len(lines) == 2 * len(items) and all(len(v) == v[0] + 1 for v in lines)
    return [(lines[2 * i][1:], lines[2 * i + 1][1:]) for i in range(len(items))]


def test_constants_are_the_host_rule(checker):
    r = subprocess.run([checker, "--constants"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L, H, D = wave_codec.PROSODY_FRAME, wave_codec.PROSODY_HOP, wave_codec.PROSODY_SEARCH
    assert [int(v) for v in r.stdout.split()] == [L, H, D, 2 * D + 1, 2 * D + L]


@pytest.mark.parametrize("stretch", STRETCHES + [(1, 1), (400, 399)], ids=lambda s: f"{s[0]}_{s[1]}")
def test_case_matrix_prints_the_host_frames_and_samples(checker, tmp_path, stretch):
    P, Q = stretch
    items = [(_content(kind, n), P, Q) for n in LENGTHS for kind in CONTENTS]
    for (x, _, _), (starts, samples) in zip(items, _run(checker, tmp_path, items)):
        y, s = wave_codec._wsola_frames(x, P, Q)
        assert starts == s and samples == y.tolist(), (len(x), stretch)


def test_a_bad_case_is_refused(checker, tmp_path):
    p = tmp_path / "bad.bin"
    p.write_bytes(struct.pack("<3i", 3, 1, 0))
    r = subprocess.run([checker, str(p)], capture_output=True, text=True)
    assert r.returncode == 2 and "refused" in r.stderr
