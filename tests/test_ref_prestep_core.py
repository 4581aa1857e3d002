"""CPU: the device pre-step's core (csrc/ref_prestep_core.h: the geometry, the integer comparisons and the sequential rule the kernels
compile) as a stand-alone program (tools/ref_prestep_check.cpp) built with the host C++ compiler under AddressSanitizer and UBSan.  It is
fed the per-millisecond sums of squares of every case (and the per-frame sums that stand in for the samples of a partial cell); every
table it reads lives in a heap block of exactly its size, so a read out of bounds is a report and a non-zero exit.  It must print the
ranges of `audio_prep.preprocess_ref_ranges`.  No Python extension and no preloaded library is involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_prestep_cases as RC
from tts_indic_server_f5_amd import audio_prep as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/ref_prestep_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("ref_prestep_check") / "ref_prestep_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "ref_prestep_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _tables(x, rate, clip_short):
    seg = AP.PcmSegment(x, rate)
    c = seg._cum_squares()
    L = len(seg)
    at = seg._frames(np.arange(L + 1, dtype=np.int64))
    return np.concatenate([np.array([seg.frames.shape[0], seg.frames.shape[1], rate, int(clip_short)], dtype=np.int64),
                           np.diff(c[at]), np.diff(c)]).astype("<i8")


def _run(checker, tmp_path, items):
    """[(ranges, tail)] of the program over (frames, rate, clip_short) items; it must exit 0 with nothing from a sanitizer."""
    files = []
    for i, (x, rate, clip) in enumerate(items):
        p = tmp_path / f"case{i}.bin"
        _tables(x, rate, clip).tofile(p)
        files.append(str(p))
    r = subprocess.run([checker] + files, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = []
    for line in r.stdout.splitlines():
        v = [int(t) for t in line.split()]
        assert len(v) == 2 * v[0] + 2
        out.append(([[v[1 + 2 * j], v[2 + 2 * j]] for j in range(v[0])], v[-1]))
    assert len(out) == len(items)
    return out


def test_constants_are_the_host_rule(checker):
    r = subprocess.run([checker, "--constants"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t1, t2, te = RC.thresholds()
    assert [int(v) for v in r.stdout.split()] == [t1, t2, te + 1]


def test_case_matrix_prints_the_host_ranges(checker, tmp_path):
    cases = RC.cases()
    got = _run(checker, tmp_path, list(cases.values()))
    for (name, (x, rate, clip)), (ranges, tail) in zip(cases.items(), got):
        want = AP.preprocess_ref_ranges(AP.PcmSegment(x, rate), clip)
        assert (ranges, tail) == (want[0], want[1]), name


def test_random_layouts_print_the_host_ranges(checker, tmp_path):
    items = [RC.random_layout(s) for s in range(60)]
    for i, ((x, rate, clip), (ranges, tail)) in enumerate(zip(items, _run(checker, tmp_path, items))):
        want = AP.preprocess_ref_ranges(AP.PcmSegment(x, rate), clip)
        assert (ranges, tail) == (want[0], want[1]), f"layout {i}"
