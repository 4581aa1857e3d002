"""Writes csrc/wsola_window.inc, the rising half of the WSOLA window the device call builds in: `wave_codec.wsola_window()[:480]` as a C
initialiser list, 16 values a line.  tests/test_prosody_host.py holds the committed file to the function, so run this after changing either.

    python tools/gen_wsola_window.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tts_indic_server_f5_amd import wave_codec  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-indic-server-f5_amd", "csrc", "wsola_window.inc")


def text():
    rise = [int(v) for v in wave_codec.wsola_window()[:wave_codec.PROSODY_HOP]]
    head = ("// wave_codec.wsola_window()[:480]: W[i] = rint(32768 sin^2(pi (2 i + 1) / 1920)), the rising half of the 960-sample WSOLA window; the\n"
            f"// falling half is 32768 - W[i].  {len(rise)} values, the largest {max(rise)}.  Written by tools/gen_wsola_window.py; tests/test_prosody_host.py\n"
            "// compares it with the function.\n")
    return head + "".join(", ".join(str(v) for v in rise[i:i + 16]) + ",\n" for i in range(0, len(rise), 16))


if __name__ == "__main__":
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(text())
    print(f"{OUT}: {wave_codec.PROSODY_HOP} values")
