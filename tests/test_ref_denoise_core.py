"""CPU: the device denoiser's geometry (csrc/ref_denoise_core.h: the frames of a clip, the rank, the smoothing window's clamp, the frame range
of a sample, the checked clip table -- the text the kernels and the host entry point compile) as a stand-alone program
(tools/ref_denoise_check.cpp) built with the host C++ compiler under AddressSanitizer and UBSan.  It walks every index the four launches form
for every clip length from 1 to 2100 and for the greatest one, over heap blocks of exactly the tables' sizes, so an index out of bounds is a
report and a non-zero exit.  No Python extension and no preloaded library is involved; the kernels themselves run under no sanitizer."""
import os
import shutil
import subprocess

import pytest

from tts_indic_server_f5_amd import audio_prep as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/ref_denoise_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("ref_denoise_check") / "ref_denoise_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "ref_denoise_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(checker, *args):
    r = subprocess.run([checker, *args], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_constants_are_the_host_definition(checker):
    v = _run(checker, "--constants").split()
    assert [int(t) for t in v[:6]] == [AP.DENOISE_N_FFT, AP.DENOISE_HOP, AP.DENOISE_PAD, AP.DENOISE_N_FFT // 2 + 1, 516, AP.DENOISE_RANK_DIV]
    assert (float(v[6]), float(v[7]), int(v[8])) == (AP.DENOISE_SUBTRACT, AP.DENOISE_MIN_GAIN, AP.DENOISE_MAX_SAMPLES)


def test_every_length_walks_inside_its_tables(checker):
    lengths = list(range(1, 2101)) + [AP.DENOISE_MAX_SAMPLES]
    lines = _run(checker, *map(str, lengths)).splitlines()
    assert len(lines) == len(lengths)
    for n, line in zip(lengths, lines):
        F = AP.denoise_frames(n)
        assert [int(t) for t in line.split()] == [n, F, (F - 1) // AP.DENOISE_RANK_DIV, 4 * n], line
    assert lines[-1].split()[1] == "5628"


def test_clip_table_and_refusals(checker):
    ok, codes = _run(checker, "--table").splitlines()
    lens, offs = [1, 2100, AP.DENOISE_MAX_SAMPLES, 257], [5000000, 10, 2000000, 2200]
    frames = [AP.denoise_frames(n) for n in lens]
    want = ["ok", str(sum(frames)), str(sum(lens))]
    for i in range(4):
        want.append(f"{sum(frames[:i])}:{frames[i]}:{sum(lens[:i])}:{offs[i]}")
    assert ok.split() == want
    # no clips, a length of 0, a length above the limit, a negative offset, two overlaps (one of them a shared start), a null table,
    # one row too many, and the greatest table that passes
    assert [int(t) for t in codes.split()] == [1, 3, 3, 4, 5, 5, 2, 6, 0]
