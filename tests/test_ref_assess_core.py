"""CPU: the reference-clip report's run rule and index geometry (csrc/ref_assess_core.h: the flat index of the raw side, the run of three
inside one channel, the 8-bin windows, the checked raw clip table -- the text the kernels and the host entry point compile) as a stand-alone
program (tools/ref_assess_check.cpp) built with the host C++ compiler under AddressSanitizer and UBSan.  Every clip lives in a heap block of
exactly its size, so a neighbour read past a channel that leaves the block is a report and a non-zero exit.  No Python extension and no
preloaded library is involved; the kernels themselves run under no sanitizer."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import assess_ref as A  # noqa: E402
from tts_indic_server_f5_amd import audio_prep as AP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/ref_assess_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("ref_assess_check") / "ref_assess_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "ref_assess_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(checker, *args):
    r = subprocess.run([checker, *args], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_constants_are_the_host_definition(checker):
    v = _run(checker, "--constants").split()
    assert [float(t) for t in v[:2]] == [AP.ASSESS_HOT, AP.ASSESS_MIN_PEAK] and int(v[2]) == AP.ASSESS_MIN_RUN
    assert (int(v[3]), int(v[4])) == AP.ASSESS_BAND
    assert [float(t) for t in v[5:8]] == [AP.ASSESS_FLOOR_TO_MEAN, AP.ASSESS_SPEECH_FACTOR, AP.ASSESS_BANDWIDTH_REL]
    assert [int(t) for t in v[8:]] == [AP.ASSESS_MEAN_BINS, 513 - AP.ASSESS_MEAN_BINS + 1, 508, AP.ASSESS_MAX_CHANNELS, 4096, len(AP.ASSESS_ROW), 16]


@pytest.mark.parametrize("name", list(A.run_cases()))
def test_run_rule_cases(checker, name):
    x, want = A.run_cases()[name]
    out = _run(checker, "--runs", str(x.shape[0]), str(x.shape[1]), *(repr(float(v)) for v in x.reshape(-1))).split()
    peak, clipped = AP.assess_clipping(x)
    assert int(out[0]) == int(np.array([peak], dtype=np.float32).view(np.uint32)[0])
    assert int(out[2]) == clipped == want


def test_run_rule_on_random_clips(checker):
    rng = np.random.default_rng(5)
    for _ in range(25):
        ch, n = int(rng.integers(1, 9)), int(rng.integers(1, 40))
        x = rng.choice(np.array([1.0, -1.0, 32767 / 32768, 0.999, 0.5, 0.0], dtype=np.float32), size=(ch, n), p=[.3, .2, .1, .1, .2, .1])
        out = _run(checker, "--runs", str(ch), str(n), *(repr(float(v)) for v in x.reshape(-1))).split()
        assert int(out[2]) == AP.assess_clipping(x)[1] == A.clipping(x)[1]


def test_every_flat_index_stays_inside_its_channel(checker):
    for ch, n in ((1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (3, 3), (8, 1), (8, 5), (2, 1000), (3, 257), (1, 100000)):
        out = [int(t) for t in _run(checker, "--walk", str(ch), str(n)).split()]
        reads = ch * sum(min(n - 1, j + 2) - max(0, j - 2) + 1 for j in range(n))            # the neighbours inside the channel, no others
        assert out == [ch, n, reads, 512], (ch, n)


def test_every_frame_row_lies_in_exactly_one_tile(checker):
    frames = list(range(1, 70)) + [AP.denoise_frames(AP.ASSESS_MAX_SAMPLES)]
    lines = _run(checker, "--tiles", *map(str, frames)).splitlines()
    for F, line in zip(frames, lines):
        assert [int(t) for t in line.split()] == [F, -(-F // 16), F - 16 * ((F - 1) // 16)], line
    assert len(lines) == len(frames)


def test_raw_clip_table_and_refusals(checker):
    ok, codes = _run(checker, "--table").splitlines()
    assert ok.split() == ["ok", "4", "5000:1000:2:2000:0", "0:1:1:1:1", "100:5:8:40:2"]          # clips of 1, 16 and 17 frames: 1, 1 and 2 tiles
    # no clips, too many, null tables, no channel, nine channels, an empty clip, more than 2^31 - 1 samples, a negative offset, two overlaps
    # (one through a second channel, one a shared start), and adjacent clips, which pass
    assert [int(t) for t in codes.split()] == [1, 1, 2, 3, 3, 4, 4, 5, 6, 6, 0]
