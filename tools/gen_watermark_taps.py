"""Writes csrc/watermark_taps.inc, the band taps the watermark's carrier is shaped with: `wave_codec.watermark_taps()` as a C initialiser
list, 16 values a line.  tests/test_watermark_host.py holds the committed file to the function, so run this after changing either.

    python tools/gen_watermark_taps.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tts_indic_server_f5_amd import wave_codec  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-indic-server-f5_amd", "csrc", "watermark_taps.inc")


def text():
    g = [int(v) for v in wave_codec.watermark_taps()]
    head = ("// wave_codec.watermark_taps(): g[k] = rint(2^14 hann[k] (2 f1 sinc(2 f1 (k - 64)) - 2 f0 sinc(2 f0 (k - 64)))), f1 = 3200 / 24000,\n"
            "// f0 = 500 / 24000, hann[k] = 0.5 - 0.5 cos(2 pi (k + 1) / 130): the 500 .. 3200 Hz band the watermark's chips are shaped with.\n"
            f"// {len(g)} values, sum {sum(g)}, sum of magnitudes {sum(abs(v) for v in g)}.  Written by tools/gen_watermark_taps.py;\n"
            "// tests/test_watermark_host.py compares it with the function.\n")
    return head + "".join(", ".join(str(v) for v in g[i:i + 16]) + ",\n" for i in range(0, len(g), 16))


if __name__ == "__main__":
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(text())
    print(f"{OUT}: {wave_codec.WATERMARK_TAPS} values")
