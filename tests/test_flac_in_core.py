"""CPU: the device FLAC decoder's core (csrc/flac_in_core.h: the bit reader and the per-frame arithmetic the kernels compile) as a stand-alone
program (tools/flac_in_check.cpp) built with the host C++ compiler under AddressSanitizer and UBSan.  Every stream lives in a heap block
of exactly its size, every slot pool and output in one of the size the library would give it, so a read or write out of bounds is a
report and a non-zero exit.  The program must agree with `wave_codec.read_flac` on the case matrix and on 2 000 damaged streams: the same
verdict, and the same samples when it accepts.  No Python extension and no preloaded library is involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import flac_cases as C
from tts_indic_server_f5_amd import wave_codec as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler on PATH: the bounds of csrc/flac_in_core.h cannot be checked"
    exe = tmp_path_factory.mktemp("flac_in_check") / "flac_in_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tools", "flac_in_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(checker, tmp_path, streams):
    """[(status, samples or None)] of the program over `streams`, which must end with exit status 0 and nothing from a sanitizer."""
    results = []
    for lo in range(0, len(streams), 500):                      # (command lines stay short)
        files = []
        for i, s in enumerate(streams[lo:lo + 500]):
            p = tmp_path / f"s{lo + i}.flac"
            p.write_bytes(s)
            files.append(str(p))
        out = tmp_path / f"out{lo}.bin"
        r = subprocess.run([checker, str(out)] + files, capture_output=True, text=True)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(files)
        data, at = np.fromfile(out, dtype=np.int32), 0
        for line in lines:
            status, count, ch = (int(v) for v in line.split())
            if status == 0:
                results.append((0, data[at:at + count * ch].reshape(ch, count)))
                at += count * ch
            else:
                results.append((status, None))
        assert at == len(data)
    return results


def _agrees(name, stream, status, samples):
    """The program's verdict on `stream` against `read_flac`'s; the MD5 is the host's check for both decoders."""
    try:
        want, err = W.read_flac(stream), None
    except ValueError as e:
        want, err = None, str(e)
    if status == 2:                                             # "needs the host": the caller runs read_flac, whatever it says
        return "host"
    if status != 0:
        assert want is None, f"{name}: the core refuses a stream that read_flac accepts"
        return "refused"
    try:
        W.flac_check_md5(samples, W.flac_stream_info(stream))
    except ValueError as e:
        assert want is None and str(e) == err, f"{name}: {err}"
        return "refused"
    assert want is not None, f"{name}: the core accepts a stream that read_flac refuses: {err}"
    assert np.array_equal(samples, want[0]), name
    return "accepted"


def test_case_matrix_equals_read_flac(checker, tmp_path):
    cases = C.cases()
    got = _run(checker, tmp_path, [v["stream"] for v in cases.values()])
    for (name, v), (status, samples) in zip(cases.items(), got):
        if v["device"]:
            assert status == 0 and np.array_equal(samples, v["x"]), name
        else:
            assert status == 2, name                            # outside the limits: not decoded, not refused
    stream, x = C.false_sync()
    (status, samples), = _run(checker, tmp_path, [stream])
    assert status == 0 and np.array_equal(samples, x)


def test_named_refusals(checker, tmp_path):
    named = C.refusals()
    for (name, stream), (status, samples) in zip(named.items(), _run(checker, tmp_path, list(named.values()))):
        with pytest.raises(ValueError):
            W.read_flac(stream)
        assert status != 0, name
        assert _agrees(name, stream, status, samples) in ("refused", "host")


def test_two_thousand_mutants_same_verdict_no_report(checker, tmp_path):
    mutants = C.mutants(2000)
    assert len(mutants) == 2000 and C.mutants(5) == mutants[:5]        # a fixed seed
    verdicts = [_agrees(f"mutant {i}", m, status, samples) for i, (m, (status, samples)) in enumerate(zip(mutants, _run(checker, tmp_path, mutants)))]
    # the corpus is neither all noise nor all intact: both verdicts occur, and few streams are handed to the host undecided
    assert verdicts.count("accepted") >= 20 and verdicts.count("refused") >= 1000 and verdicts.count("host") <= 100, \
        {v: verdicts.count(v) for v in set(verdicts)}
