"""Writes csrc/loudness_taps.inc, the K-weighting tap table the device meter builds in: `wave_codec.loudness_taps()` as a C initialiser
list, 16 values a line.  tests/test_loudness_host.py holds the committed file to the function, so run this after changing either.

    python tools/gen_loudness_taps.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tts_indic_server_f5_amd import wave_codec  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts-indic-server-f5_amd", "csrc", "loudness_taps.inc")


def text():
    taps = [int(v) for v in wave_codec.loudness_taps()]
    head = ("// wave_codec.loudness_taps(): rint(2^16 k_true[k]), k_true the impulse response of the two K-weighting biquads of BS.1770 designed for\n"
            f"// 24 kHz; {len(taps)} taps, sum |h| = {sum(abs(v) for v in taps)}.  Written by tools/gen_loudness_taps.py; tests/test_loudness_host.py compares it with the function.\n")
    return head + "".join(", ".join(str(v) for v in taps[i:i + 16]) + ",\n" for i in range(0, len(taps), 16))


if __name__ == "__main__":
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(text())
    print(f"{OUT}: {len(wave_codec.loudness_taps())} taps")
