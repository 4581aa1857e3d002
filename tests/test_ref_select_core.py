"""CPU: the reference-stretch selection's radix select, window geometry, source buckets and row arithmetic (csrc/ref_select_core.h, the text
the kernels and the host entry point compile) as a stand-alone program (tools/ref_select_check.cpp) built with the host C++ compiler under
AddressSanitizer and UBSan.  The stage, the candidate list and the bin column live in heap blocks of exactly the kernel's sizes and a
workgroup's walk is replayed read for read, so an index past one of them is a report and a non-zero exit.  No Python extension and no
preloaded library is involved; the kernels themselves run under no sanitizer."""
import os
import shutil
import subprocess

import pytest

from tts_indic_server_f5_amd import audio_prep as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/ref_select_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("ref_select_check") / "ref_select_check"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                        os.path.join(ROOT, "tools", "ref_select_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(checker, *args):
    r = subprocess.run([checker, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_constants_rows_and_table(checker):
    assert [int(t) for t in _run(checker, "--constants").split()] == [AP.SELECT_MAX_SAMPLES, AP.SELECT_HOP, AP.select_window_frames(15.0) + 1, 339, 340, 4096, 16, 5, 32]
    snr, keys = _run(checker, "--rows").splitlines()
    assert [float(t) for t in snr.split()] == [AP.assess_ratios(n, s, 0, 1, -1)["snr_db"] for n, s in ((0.0, 1.0), (1.0, 1.0), (1.0, 11.0), (0.0, 0.0))]
    assert keys.split() == ["1", "1", "0", "1", "0", "0"]
    ok, codes = _run(checker, "--table").splitlines()
    # recordings of 103, 4 and 34 frames at W 20, hop 4: 21, 1 (short) and 4 windows in 2, 1 and 1 runs of 16
    assert ok.split() == ["ok", "141", "48816", "26", "4", "7", "135", "16", "103:104:20:21:0:0:2:100:0", "4:4:4:1:21:2:1:1:101", "34:36:20:4:22:3:1:31:103"]
    assert [int(t) for t in codes.split()] == [1, 1, 2, 3, 3, 4, 5, 6, 6, 7, 8, 0, 9, 0]


# W, hop, F, seed: the suite's shapes, the widest window at hop 1 and at the default hop, a column longer than the stage (96 s: every
# workgroup stages its own range of it), a hop past the window, a short recording, ties
@pytest.mark.parametrize("W,hop,F,seed", [(20, 4, 85, 7), (1125, 48, 1941, 3), (1407, 1, 1500, 4), (1407, 48, 2900, 5), (1407, 48, 9001, 5), (5, 9, 200, 6), (93, 48, 60, 5),
                                          (1, 1, 40, 1), (20, 4, 100, 0), (93, 48, 1000, 1)])
def test_every_window_of_every_workgroup_picks_the_sorted_element(checker, W, hop, F, seed):
    lines = _run(checker, "--select", W, hop, F, seed).splitlines()
    assert len(lines) == len(AP.select_windows(F, W, hop))                       # (the program exits 3 at the first window that differs)


@pytest.mark.parametrize("length,sr,n", [(10000, 44100, 20000), (10000, 8000, 3400), (257, 24000, 300), (1, 48000, 5), (256 * 40, 11025, 4704)])
def test_every_raw_sample_lies_in_its_bucket_or_past_the_end(checker, length, sr, n):
    nb, inside, outside = (int(t) for t in _run(checker, "--buckets", length, sr, n).split())
    end = length * sr // 24000
    assert nb == -(-length // 256) and inside == min(n, end) and outside == n - inside
