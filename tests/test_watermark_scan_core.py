"""CPU: the watermark scan's range arithmetic (csrc/wave_mark_core.h: the segments of a recording, a range's first sample and sample
count, the zero fill past the end, the four frames that hold a sample, the slab rule) as a stand-alone program
(tools/watermark_scan_check.cpp) built with the host C++ compiler under AddressSanitizer and UBSan.  It runs ws_range_fold_kernel's threads
serially with the frames in a heap block of exactly their size, so a read out of bounds is a report and a non-zero exit, and prints what
each residue reads; this test equates that with the definition written above `wave_codec.scan_watermark`.  No Python extension and no
preloaded library is involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tts_indic_server_f5_amd import wave_codec
from tts_indic_server_f5_amd.wave_codec import WATERMARK_SCAN_WINDOW  # noqa: F401  (the scan's constants: absent before it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = wave_codec.WATERMARK_PERIOD
N_FFT, HOP, PAD = 1024, 256, 768
LENGTHS = (1, 255, 12000, P - 1, P, P + 1, 5 * P + 1000)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/wave_mark_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("watermark_scan_check") / "watermark_scan_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "watermark_scan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _ranges(n):
    """The first segment, the last (partial) one, a single one in the middle and the whole recording, without repeats."""
    S = -(-n // P)
    return sorted({(0, 1), (S - 1, 1), (S // 2, 1), (0, S), (max(S - 2, 0), min(2, S))})


def _frames_of(j, F):
    """[(frame, position)] of sample j by the definition: frame f holds samples 256 f - 768 .. 256 f + 255."""
    found = [(f, j - (HOP * f - PAD)) for f in range(max(0, j // HOP - 6), j // HOP + 7) if HOP * f - PAD <= j <= HOP * f + HOP - 1]
    assert len(found) == N_FFT // HOP and found[-1][0] < F and all(0 <= o < N_FFT for _, o in found), (j, found)
    return found


def _residues(n):
    tail = n % P
    return sorted({m for m in (0, 1, 255, 256, 257, 999, 1000, 1001, 11999, P - 2, P - 1, tail - 1, tail, tail + 1) if 0 <= m < P})


def test_constants_and_slabs(checker):
    r = subprocess.run([checker, "--constants"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in r.stdout.split()] == [wave_codec.WATERMARK_SCAN_WINDOW, wave_codec.WATERMARK_SCAN_SLACK, wave_codec.WATERMARK_SCAN_MAX_SAMPLES,
                                                  4096, 4096, N_FFT, HOP, PAD]
    for ranges, rows in ((1, 1), (878, 4), (878, 16), (4096, 16), (4096, 1), (257, 16), (256, 16), (1025, 4), (342, 12)):
        r = subprocess.run([checker, "--slabs", str(ranges), str(rows)], capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr
        per = 4096 // rows
        assert [int(v) for v in r.stdout.split()] == [per, -(-ranges // per)]
        assert per * rows * P * 4 <= 256 << 20                                          # a slab of correlations stays within 256 MiB
    for bad in (("0", "1"), ("4097", "1"), ("1", "0"), ("1", "17")):
        assert subprocess.run([checker, "--slabs", *bad], capture_output=True, text=True).returncode == 2


@pytest.mark.parametrize("n", LENGTHS)
def test_ranges_read_what_the_definition_says(checker, n):
    S, F = -(-n // P), -(-(n + PAD) // HOP)
    for first, count in _ranges(n):
        residues = _residues(n)
        r = subprocess.run([checker, str(n), str(first), str(count)] + [str(m) for m in residues], capture_output=True, text=True)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.splitlines()
        samples = min(n, (first + count) * P) - first * P
        assert lines[0].split() == [str(S), str(F), str(samples)], (n, first, count)
        # every residue: the samples s P + m of the range's segments that lie below n, each in its four frames
        j = np.arange(first * P, first * P + samples, dtype=np.int64)
        f = (j // HOP)[:, None] + np.arange(N_FFT // HOP)[None]
        o = j[:, None] + PAD - HOP * f
        assert f.max() < F and o.min() >= 0 and o.max() < N_FFT
        weight = ((j % P + 1)[:, None] * (1024 * f + o)).astype(np.uint64)
        Z = np.zeros(P)
        np.add.at(Z, j % P, ((7 * f + 3 * o) % 11).sum(axis=1))
        fold = float(((np.arange(P) % 13 + 1) * Z).sum())
        assert lines[1].split() == [str(f.size), str(int(weight.sum(dtype=np.uint64))), f"{fold:.0f}"], (n, first, count)
        for line, m in zip(lines[2:], residues):
            want = f"{m}:"
            for s in range(first, first + count):
                if s * P + m < n:                                                       # at or past n: the zero fill, not read
                    want += f" {s * P + m}" + "".join(f" {fr}:{pos}" for fr, pos in _frames_of(s * P + m, F)) + ";"
            assert line == want, (n, first, count, m)
        assert len(lines) == 2 + len(residues)


def test_a_bad_range_is_refused(checker):
    for n, first, count in ((0, 0, 1), (wave_codec.WATERMARK_SCAN_MAX_SAMPLES + 1, 0, 1), (P, 1, 1), (P + 1, 0, 3), (P, 0, 0), (P, -1, 1), (5 * P, 5, 1)):
        r = subprocess.run([checker, str(n), str(first), str(count)], capture_output=True, text=True)
        assert r.returncode == 2 and "refused" in r.stderr, (n, first, count)
    r = subprocess.run([checker, str(wave_codec.WATERMARK_SCAN_MAX_SAMPLES), "0", "879", "0", str(P - 1)], capture_output=True, text=True)   # the cap, whole
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and r.stdout.splitlines()[0].split() == ["879", "56253", str(wave_codec.WATERMARK_SCAN_MAX_SAMPLES)]
