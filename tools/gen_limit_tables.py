"""Writes the two tables the true-peak limiter's device call builds in, as C initialiser lists: csrc/truepeak_taps.inc
(`wave_codec.truepeak_taps()`, three phases of 12 taps, a phase a line) and csrc/limit_window.inc (`wave_codec.limit_window()`, 481 weights,
16 a line).  tests/test_limit_host.py holds the committed files to the functions, so run this after changing either.

    python tools/gen_limit_tables.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tts_indic_server_f5_amd import wave_codec  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-indic-server-f5_amd", "csrc")


def taps_text():
    taps = wave_codec.truepeak_taps()
    head = ("// wave_codec.truepeak_taps(): phase p = 1, 2, 3 of the 4x true-peak interpolator, t[p][k] = rint(2^14 c_k / sum c) with c_k = sinc(d)\n"
            "// I0(5 sqrt(1 - (d / 6)^2)) / I0(5) at d = k - 5 - p / 4: the point i + p / 4 from x[i - 5 .. i + 6].  The largest sum |t[p]| is\n"
            f"// {int(abs(taps).sum(axis=1).max())}.  Written by tools/gen_limit_tables.py; tests/test_limit_host.py compares it with the function.\n")
    return head + "".join(", ".join(str(int(v)) for v in row) + ",\n" for row in taps)


def window_text():
    w = [int(v) for v in wave_codec.limit_window()]
    head = ("// wave_codec.limit_window(): w[k] = rint(2^16 (1 + cos(pi k / 241)) / 482) for k = -240 .. 240, the centre raised so that the 481 weights\n"
            f"// sum to exactly 2^16; the largest is {max(w)}.  Written by tools/gen_limit_tables.py; tests/test_limit_host.py compares it with the function.\n")
    return head + "".join(", ".join(str(v) for v in w[i:i + 16]) + ",\n" for i in range(0, len(w), 16))


if __name__ == "__main__":
    for name, text in (("truepeak_taps.inc", taps_text()), ("limit_window.inc", window_text())):
        with open(os.path.join(CSRC, name), "w", encoding="utf-8") as f:
            f.write(text)
        print(os.path.join(CSRC, name))
