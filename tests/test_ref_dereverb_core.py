"""CPU: the device dereverberator's geometry (csrc/ref_dereverb_core.h: the staged chunk of a bin's delay line, the power window of lam, the
chunking of a clip's frames, the checked clip table -- the text the kernel and the host entry point compile) as a stand-alone program
(tools/ref_dereverb_check.cpp) built with the host C++ compiler under AddressSanitizer and UBSan.  It forms every index the WPE kernel forms
for the lengths around each change of path and for the greatest one, over heap blocks of exactly the tables' sizes, so an index out of bounds
is a report and a non-zero exit.  No Python extension and no preloaded library is involved; the kernels themselves run under no sanitizer."""
import os
import shutil
import subprocess

import pytest

from tts_indic_server_f5_amd import audio_prep as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, K, CHUNK = AP.DEREVERB_DELAY, AP.DEREVERB_TAPS, 128


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/ref_dereverb_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("ref_dereverb_check") / "ref_dereverb_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "ref_dereverb_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(checker, *args):
    r = subprocess.run([checker, *args], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_constants_are_the_host_definition(checker):
    v = _run(checker, "--constants").split()
    assert [int(t) for t in v[:10]] == [D, K, AP.DEREVERB_ITERATIONS, CHUNK, D + K - 1, CHUNK + D + K - 1, CHUNK + 2, 8, 65, 2 * K]
    assert [float(t) for t in v[10:]] == [AP.DEREVERB_FLOOR, AP.DEREVERB_LOAD, AP.DEREVERB_TINY]


def test_lengths_around_every_change_of_path_walk_inside_their_tables(checker):
    frames = [4, 5, D + K - 1, D + K, D + K + 1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + D + K, 2 * CHUNK, 2 * CHUNK + 1, 3 * CHUNK - 1]
    lengths = [1] + [256 * F - 768 - d for F in frames for d in (255, 0)] + [AP.DENOISE_MAX_SAMPLES]
    lines = _run(checker, *map(str, lengths)).splitlines()
    assert len(lines) == len(lengths)
    for n, line in zip(lengths, lines):
        F = AP.denoise_frames(n)
        assert [int(t) for t in line.split()] == [n, F, -(-F // CHUNK), sum(min(max(f - D + 1, 0), K) for f in range(F))], line
    assert lines[-1].split()[1:3] == ["5628", "44"]


def test_clip_table_and_refusals(checker):
    ok, codes = _run(checker, "--table").splitlines()
    lens, offs = [1, AP.DEREVERB_MAX_SAMPLES, 32257], [5000000, 10, 2000000]
    frames = [AP.denoise_frames(n) for n in lens]
    assert ok.split() == ["ok", str(sum(frames)), str(sum(lens))] + [f"{sum(frames[:i])}:{frames[i]}:{sum(lens[:i])}:{offs[i]}" for i in range(3)]
    # no clips, a length of 0, a length above the limit, a negative offset, an overlap, a null table, one workgroup too many, and a table that passes
    assert [int(t) for t in codes.split()] == [1, 3, 3, 4, 5, 2, 6, 0]
