"""CPU: the watermark's core (csrc/wave_mark_core.h: the carrier, the tile and block geometry, the masked block sums, the envelope and the
sample arithmetic the kernels compile) as a stand-alone program (tools/wave_mark_check.cpp) built with the host C++ compiler under
AddressSanitizer and UBSan.  It runs the two launches of f5hip_wave_mark serially -- every block sum of every tile, then the groups of 8
samples -- with the samples, the block sums, the chips and the carrier each in a heap block of exactly its size, so a read or write out of
bounds is a report and a non-zero exit.  It must print the digests and the samples of `wave_codec.mark_pcm16`.  No Python extension and no
preloaded library is involved."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tts_indic_server_f5_amd import wave_codec

from test_watermark_host import _content

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 32 * 240
LENGTHS = (0, 1, 7, 8, 239, 240, 241, 480, TILE - 1, TILE, TILE + 1, 16383, 16384, 16385, 40000)
KEYS = (1, 0xDEADBEEF, 2 ** 48 - 1)


def _fnv1a(pcm):
    h = 0xCBF29CE484222325
    for byte in np.ascontiguousarray(pcm, dtype="<i2").tobytes():
        h = ((h ^ byte) * 0x100000001B3) & (2 ** 64 - 1)
    return h


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/wave_mark_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("wave_mark_check") / "wave_mark_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "wave_mark_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(checker, tmp_path, items):
    """[(n, digest, changed, first samples)] of the program over (x, key, len) items; it must exit 0 with nothing from a sanitizer."""
    files = []
    for i, (x, key, length) in enumerate(items):
        p = tmp_path / f"case{i}.bin"
        p.write_bytes(struct.pack("<Q2i", key, len(x), length) + x.astype("<i2").tobytes())
        files.append(str(p))
    r = subprocess.run([checker] + files, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = [[int(t) for t in line.split()] for line in r.stdout.splitlines()]
    assert len(lines) == len(items)
    return [(v[0], v[1], v[2], v[3:]) for v in lines]


def test_constants_are_the_host_rule(checker):
    r = subprocess.run([checker, "--constants"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in r.stdout.split()] == [wave_codec.WATERMARK_PERIOD, wave_codec.WATERMARK_BLOCK, wave_codec.WATERMARK_TAPS,
                                                  wave_codec.WATERMARK_SHIFT, 32, TILE, wave_codec.WATERMARK_KEYS_MAX, *wave_codec.WATERMARK_BAND,
                                                  wave_codec.WATERMARK_MIN_SAMPLES]


@pytest.mark.parametrize("key", KEYS)
def test_carrier_is_the_host_carrier(checker, key):
    r = subprocess.run([checker, "--carrier", str(key)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr
    c = wave_codec.watermark_carrier(key)
    c64 = c.astype(np.int64)
    assert [int(v) for v in r.stdout.split()] == [int(c64.sum()), int((c64 * c64).sum()), int(c.min()), int(c.max()), _fnv1a(c)] + c[:16].tolist()


@pytest.mark.parametrize("kind", ["speech", "full", "noise"])
def test_case_matrix_prints_the_host_samples(checker, tmp_path, kind):
    items = [(_content(kind, n) if n else np.zeros(0, dtype=np.int16), key, n) for n in LENGTHS for key in KEYS[:2]]
    items += [(_content(kind, n), 1, length) for n, length in ((481, 240), (TILE + 1, TILE), (16385, 1), (40000, 0), (40000, 16384))]   # a device length below the bound
    for (x, key, length), (n, digest, changed, first) in zip(items, _run(checker, tmp_path, items)):
        want = np.concatenate([wave_codec.mark_pcm16(x[:length], key), x[length:]])     # samples past the length keep their bits
        assert n == len(x) and digest == _fnv1a(want) and changed == int((want != x).sum()) and first == want[:64].tolist(), (kind, len(x), key, length)


def test_silence_and_zero_blocks(checker, tmp_path):
    x = _content("speech", 40000).copy()
    x[10000:20000] = 0
    items = [(np.zeros(20000, dtype=np.int16), 1, 20000), (x, 1, 40000)]
    (n0, d0, changed0, _), (n1, d1, _, _) = _run(checker, tmp_path, items)
    assert changed0 == 0 and d0 == _fnv1a(items[0][0])                                  # zeros stay zeros
    assert d1 == _fnv1a(wave_codec.mark_pcm16(x, 1))


def test_a_bad_case_is_refused(checker, tmp_path):
    for i, (key, n, length) in enumerate(((0, 0, 0), (2 ** 48, 0, 0), (1, 4, 5), (1, -1, 0))):
        p = tmp_path / f"bad{i}.bin"
        p.write_bytes(struct.pack("<Q2i", key, n, length) + b"\0" * (2 * max(n, 0)))
        r = subprocess.run([checker, str(p)], capture_output=True, text=True)
        assert r.returncode == 2 and "refused" in r.stderr, (key, n, length)
