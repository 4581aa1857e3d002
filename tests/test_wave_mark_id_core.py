"""CPU: the trace ids of the watermark's core (csrc/wave_mark_core.h: the symbols of an id, the rotated sub-key rows, the combined-carrier
sample arithmetic and the candidate offsets the kernels compile) as a stand-alone program (tools/wave_mark_id_check.cpp) built with the host
C++ compiler under AddressSanitizer and UBSan.  It runs the two launches of f5hip_wave_mark_ids serially -- every block sum of every tile,
then the groups of 8 samples over the key's row and the three rotated sub-key rows -- with the samples, the block sums and each carrier row
in a heap block of exactly its size, so a read or write out of bounds is a report and a non-zero exit.  It must print the digests and the
samples of `wave_codec.mark_pcm16` for a `WatermarkTag`.  No Python extension and no preloaded library is involved."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tts_indic_server_f5_amd import wave_codec

from test_watermark_host import _content
from test_wave_mark_core import _fnv1a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 32 * 240
LENGTHS = (0, 1, 7, 8, 239, 240, 241, 480, TILE - 1, TILE, TILE + 1, 16383, 16384, 16385, 40000)
KEYS = (1, 0xDEADBEEF)
IDS = (0, 2 ** 30 - 1, 1, 1023, 1024, (1023 << 20) | 1, 0x2A5F3C91)      # symbols 0, 1 and 1023 in each position, and a mixed one


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/wave_mark_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("wave_mark_id_check") / "wave_mark_id_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "wave_mark_id_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _mark(key, tag):
    return key if tag < 0 else wave_codec.WatermarkTag(key, tag)


def _run(checker, tmp_path, items):
    """[(n, digest, changed, first samples)] of the program over (x, key, id, len) items; it must exit 0 with nothing from a sanitizer."""
    files = []
    for i, (x, key, tag, length) in enumerate(items):
        p = tmp_path / f"case{i}.bin"
        p.write_bytes(struct.pack("<Q3i", key, tag, len(x), length) + x.astype("<i2").tobytes())
        files.append(str(p))
    r = subprocess.run([checker] + files, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = [[int(t) for t in line.split()] for line in r.stdout.splitlines()]
    assert len(lines) == len(items)
    return [(v[0], v[1], v[2], v[3:]) for v in lines]


def test_constants_and_subkeys_are_the_host_rule(checker):
    r = subprocess.run([checker, "--constants"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in r.stdout.split()] == [wave_codec.WATERMARK_ID_SYMBOLS, wave_codec.WATERMARK_ID_STEP, 10, wave_codec.WATERMARK_ID_MAX,
                                                  wave_codec.WATERMARK_ID_SHIFT, 4, wave_codec.WATERMARK_ID_KEYS_MAX, 10]
    for key in (1, 0xDEADBEEF, 2 ** 48 - 1):
        r = subprocess.run([checker, "--subkeys", str(key)], capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr
        assert [int(v) for v in r.stdout.split()] == wave_codec.watermark_subkeys(key)
    assert subprocess.run([checker, "--subkeys", "0"], capture_output=True, text=True).returncode == 2


def test_candidate_offsets_are_the_host_grid(checker):
    for o, s in ((0, 0), (0, 1), (0, 1023), (15, 1), (16383, 1023), (9979, 512)):
        r = subprocess.run([checker, "--grid", str(o), str(s)], capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr
        assert int(r.stdout) == (o - wave_codec.WATERMARK_ID_STEP * s) % wave_codec.WATERMARK_PERIOD
    assert subprocess.run([checker, "--grid", "0", "1024"], capture_output=True, text=True).returncode == 2


@pytest.mark.parametrize("kind", ["speech", "full", "noise"])
def test_case_matrix_prints_the_host_samples(checker, tmp_path, kind):
    items = [(_content(kind, n) if n else np.zeros(0, dtype=np.int16), KEYS[i % 2], IDS[i % len(IDS)], n) for i, n in enumerate(LENGTHS)]
    items += [(_content(kind, 40000), 1, tag, 40000) for tag in IDS]
    items += [(_content(kind, n), 1, -1, n) for n in (241, TILE + 1, 16385)]                         # a key alone: f5hip_wave_mark's bytes
    items += [(_content(kind, n), 1, 0x2A5F3C91, length) for n, length in ((481, 240), (TILE + 1, TILE), (16385, 1), (40000, 0), (40000, 16384))]
    for (x, key, tag, length), (n, digest, changed, first) in zip(items, _run(checker, tmp_path, items)):
        want = np.concatenate([wave_codec.mark_pcm16(x[:length], _mark(key, tag)), x[length:]])     # samples past the length keep their bits
        assert n == len(x) and digest == _fnv1a(want) and changed == int((want != x).sum()) and first == want[:64].tolist(), (kind, len(x), key, tag, length)


def test_silence_and_zero_blocks(checker, tmp_path):
    x = _content("speech", 40000).copy()
    x[10000:20000] = 0
    items = [(np.zeros(20000, dtype=np.int16), 1, 12345, 20000), (x, 1, 12345, 40000)]
    (n0, d0, changed0, _), (n1, d1, _, _) = _run(checker, tmp_path, items)
    assert changed0 == 0 and d0 == _fnv1a(items[0][0])                                               # zeros stay zeros
    assert d1 == _fnv1a(wave_codec.mark_pcm16(x, wave_codec.WatermarkTag(1, 12345)))


def test_a_bad_case_is_refused(checker, tmp_path):
    for i, (key, tag, n, length) in enumerate(((0, 0, 0, 0), (1, -2, 0, 0), (1, 2 ** 30, 0, 0), (1, 0, 4, 5), (1, 0, -1, 0))):
        p = tmp_path / f"bad{i}.bin"
        p.write_bytes(struct.pack("<Q3i", key, tag, n, length) + b"\0" * (2 * max(n, 0)))
        r = subprocess.run([checker, str(p)], capture_output=True, text=True)
        assert r.returncode == 2 and "refused" in r.stderr, (key, tag, n, length)
