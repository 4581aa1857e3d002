"""Writes csrc/psola_window.inc, the master Hann table of the formant-preserving pitch shift that the device call builds in:
`wave_codec.psola_window()` as a C initialiser list, 16 values a line.  tests/test_formant_host.py holds the committed file to the function
and to the fp64 formula, so run this after changing either.

    python tools/gen_psola_window.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tts_indic_server_f5_amd import wave_codec  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-indic-server-f5_amd", "csrc", "psola_window.inc")


def text():
    table = [int(v) for v in wave_codec.psola_window()]
    head = ("// wave_codec.psola_window(): M[j] = rint(32768 (1 + cos(pi j / 1024)) / 2), j = 0 .. 1024; a grain of period T weighs offset k by\n"
            f"// M[(|k| 1024) / T].  {len(table)} values, the last non-zero one at {max(j for j, v in enumerate(table) if v)}.  Written by "
            "tools/gen_psola_window.py;\n// tests/test_formant_host.py compares it with the function.\n")
    return head + "".join(", ".join(str(v) for v in table[i:i + 16]) + ",\n" for i in range(0, len(table), 16))


if __name__ == "__main__":
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(text())
    print(f"{OUT}: {wave_codec.PSOLA_TABLE + 1} values")
