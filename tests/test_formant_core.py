"""CPU: the core of the formant-preserving pitch shift (csrc/wave_formant_core.h: the geometry, the lag rule, the tie rules, the mark chain
and the blend the three kernels compile) as a stand-alone program (tools/wave_formant_check.cpp) built with the host C++ compiler under
AddressSanitizer and UBSan.  It runs the three launches serially -- tile staging and frame sums, the mark chain that hands out the synthesis
marks, the grain gather and the 64-bit divide per output tile -- with the samples, a tile's staged samples, the track, both mark lists (at
the sizes the call reserves), a tile's grains and the output each in a heap block of exactly its size, so a read or write out of bounds is a
report and a non-zero exit.  It must print the track, the marks and the samples of `wave_codec.psola_pcm16`.  No Python extension and no
preloaded library is involved."""
import os
import shutil
import struct
import subprocess

import pytest

from tts_indic_server_f5_amd import wave_codec

from test_formant_host import CONTENTS, LENGTHS, STEPS, content

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/wave_formant_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("wave_formant_check") / "wave_formant_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "wave_formant_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(checker, tmp_path, items):
    """Per (x, steps) item the program's lists: two of the track, then six per step; it must exit 0 with nothing from a sanitizer."""
    files = []
    for i, (x, steps) in enumerate(items):
        p = tmp_path / f"case{i}.bin"
        p.write_bytes(struct.pack(f"<{len(steps) + 2}i", len(steps), *steps, len(x)) + x.astype("<i2").tobytes())
        files.append(str(p))
    r = subprocess.run([checker] + files, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = [[int(t) for t in line.split()] for line in r.stdout.splitlines()]
    assert len(lines) == sum(2 + 6 * len(steps) for _, steps in items) and all(len(v) == v[0] + 1 for v in lines)
    lines = iter(v[1:] for v in lines)
    return [([next(lines), next(lines)], [[next(lines) for _ in range(6)] for _ in steps]) for _, steps in items]


def test_constants_are_the_host_rule(checker):
    r = subprocess.run([checker, "--constants"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = [wave_codec.PSOLA_HOP, wave_codec.PSOLA_WINDOW, wave_codec.PSOLA_LAG_MIN, wave_codec.PSOLA_LAG_MAX, wave_codec.PSOLA_MIN_ADVANCE,
            wave_codec.PSOLA_TABLE, min(wave_codec.PSOLA_LAG_MIN * q // p for p, q in wave_codec.PITCH_RATIOS.values())]
    got = [int(v) for v in r.stdout.split()]
    assert got[:7] == want
    frames, span, tile, grains = got[7:]
    assert span == 120 * (frames - 1) + 400 + 480 and grains == (tile + 799) // 33 + 1


@pytest.mark.parametrize("kind", CONTENTS)
def test_case_matrix_prints_the_host_marks_and_samples(checker, tmp_path, kind):
    """Every length and all twelve steps of one content: the host function's track, analysis marks, synthesis marks and samples."""
    items = [(content(kind, n), STEPS) for n in LENGTHS]
    for (x, steps), (track, per_step) in zip(items, _run(checker, tmp_path, items)):
        n = len(x)
        lag, voiced = wave_codec.psola_track(x)
        a, T, v = wave_codec.psola_marks(x, lag, voiced)
        assert track == [lag.tolist(), voiced.astype(int).tolist()], (kind, n)
        for s, got in zip(steps, per_step):
            u, idx = wave_codec.psola_synthesis(a, T, v, n, s)
            assert got[:5] == [a.tolist(), T.tolist(), v.tolist(), u.tolist(), idx.tolist()], (kind, n, s)
            assert got[5] == wave_codec.psola_pcm16(x, s).tolist(), (kind, n, s)


def test_a_bad_case_is_refused(checker, tmp_path):
    for pitch, n in ((0, 0), (7, 0), (1, -1)):
        p = tmp_path / "bad.bin"
        p.write_bytes(struct.pack("<3i", 1, pitch, n))
        r = subprocess.run([checker, str(p)], capture_output=True, text=True)
        assert r.returncode == 2 and "refused" in r.stderr
