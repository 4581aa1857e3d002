"""The case matrix of the FLAC-in tests, written by `flac_ref` (what is told, not what is good): every stream is a few frames of 16 .. 192
samples at the extremes of the format, plus one full-size case.  `cases()` builds them once per process; tests/test_flac_in_host.py reads
them with `wave_codec.read_flac`, tests/test_flac_in_core.py with the CPU build of the device core, tests/test_gpu_flac_in.py on the device."""
from __future__ import annotations

import functools

import numpy as np

import flac_ref as R

FULL = "full_size_stereo_44k1_block4096_lpc8"


def _walk(rng, ch, n, bits, step=None):
    """A bounded random walk inside `bits`: smooth enough for predictors, with noise on top."""
    top = (1 << (bits - 1)) - 1
    step = step or max(top // 64, 1)
    x = np.cumsum(rng.integers(-step, step + 1, size=(ch, n)), axis=1)
    return np.clip(x, -(top // 2), top // 2).astype(np.int64)


def _speech_like(rng, ch, n, rate, amp=9000):
    t = np.arange(n) / rate
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t)
    phase = 2 * np.pi * np.cumsum(f0) / rate
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 2.3 * t)
    out = []
    for c in range(ch):
        v = sum(np.sin((h + 1) * phase + c * 0.3) / (h + 1) for h in range(8))
        out.append(np.rint(amp * env * v / 2.0 + rng.standard_normal(n) * 40).astype(np.int64))
    return np.stack(out)


def full_size(seconds=1.0, seed=7):
    """(stream, samples): stereo 44.1 kHz 16 bit, block 4096, LPC order 8, mid/side -- the benchmark's workload at `seconds`."""
    rng = np.random.default_rng(seed)
    rate, n = 44100, int(44100 * seconds)
    x = _speech_like(rng, 2, n, rate)
    coefs = [7300, -6200, 1900, -500, 1300, -2100, 1500, -400]       # a fixed order-8 predictor at shift 12 (near the order-3 binomial, damped)
    last = n % 4096

    def subs(i, c):
        full = (i + 1) * 4096 <= n
        return R.sub("lpc", coefs=coefs, precision=14, shift=12, porder=4 if full else (2 if last % 4 == 0 and last // 4 >= 8 else 0))

    stream, sizes = R.write_flac(x, rate, 16, block=4096, subs=subs, stereo=10)
    return stream, x, sizes


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(stream, x, rate, bits, sizes: [bytes of the metadata, bytes of each frame], device: inside the device decoder's limits)."""
    rng = np.random.default_rng(2024)
    out = {}

    def add(name, x, rate, bits, **kw):
        x = np.atleast_2d(np.asarray(x, dtype=np.int64))
        stream, sizes = R.write_flac(x, rate, bits, **kw)
        blocks = kw.get("blocks") or [kw.get("block", 4096)]
        assert name not in out
        out[name] = dict(stream=stream, x=x, rate=rate, bits=bits, sizes=sizes,
                         device=x.shape[0] <= 2 and 8 <= bits <= 24 and max(blocks) <= 16384)

    # subframe types
    add("constant", np.full(96, -1234), 24000, 16, block=32, subs=[R.sub("constant")])
    add("verbatim", _walk(rng, 1, 100, 16), 24000, 16, block=32)
    for o in range(5):
        add(f"fixed_{o}", _walk(rng, 1, 100, 16), 24000, 16, blocks=[32, 32, 32, 4], subs=[R.sub("fixed", order=o)])
    # LPC order, precision, shift
    add("lpc_order_1", _walk(rng, 1, 96, 16), 16000, 16, block=48, subs=[R.sub("lpc", coefs=[15], precision=5, shift=4)])
    add("lpc_order_8", _walk(rng, 1, 192, 16), 16000, 16, block=64,
        subs=[R.sub("lpc", coefs=[900, -300, 100, -50, 20, -10, 5, -2], precision=11, shift=10, porder=2)])
    add("lpc_order_32", _walk(rng, 1, 384, 16), 16000, 16, block=192,
        subs=[R.sub("lpc", coefs=[int(v) for v in rng.integers(-40, 41, size=32)], precision=8, shift=7, porder=1)])
    add("lpc_precision_2_shift_0", _walk(rng, 1, 64, 16), 8000, 16, block=32, subs=[R.sub("lpc", coefs=[1, -2, 1], precision=2, shift=0)])
    add("lpc_precision_15_shift_14", _walk(rng, 1, 64, 16), 8000, 16, block=32, subs=[R.sub("lpc", coefs=[16383, -16384, 9000], precision=15, shift=14)])
    # Rice parameters and escapes
    add("rice_0", rng.integers(-1, 2, size=(1, 64)), 8000, 16, block=32, subs=[R.sub("fixed", order=0, params=0)])
    add("rice_14", rng.integers(-30000, 30000, size=(1, 64)), 8000, 16, block=32, subs=[R.sub("fixed", order=0, params=14)])
    add("rice_method1_30", rng.integers(-(1 << 22), 1 << 22, size=(1, 64)), 8000, 24, block=32, subs=[R.sub("fixed", order=0, method=1, params=30)])
    add("rice_method1_5", _walk(rng, 1, 64, 16, step=40), 8000, 16, block=32, subs=[R.sub("fixed", order=1, method=1, params=5, porder=1)])
    add("escape_0", (np.arange(64) * 3 - 50)[None], 8000, 16, block=32, subs=[R.sub("fixed", order=2, params=("esc", 0))])
    add("escape_17", rng.integers(-60000, 60000, size=(1, 64)), 8000, 20, block=32, subs=[R.sub("fixed", order=0, method=1, porder=1, params=[("esc", 17), 15])])
    # partition orders
    add("partition_0", _walk(rng, 1, 128, 16), 8000, 16, block=64, subs=[R.sub("fixed", order=2, porder=0)])
    add("partition_largest", _walk(rng, 1, 128, 16), 8000, 16, block=64, subs=[R.sub("fixed", order=1, porder=6)])
    add("partition_5_order_2", _walk(rng, 1, 128, 16), 8000, 16, block=64, subs=[R.sub("fixed", order=2, porder=5)])
    # wasted bits
    add("wasted_1", _walk(rng, 1, 64, 15) * 2, 8000, 16, block=32, subs=[R.sub("fixed", order=2, wasted=1)])
    add("wasted_7", _walk(rng, 2, 64, 9) * 128, 8000, 16, block=32, subs=[R.sub("lpc", coefs=[2, -1], precision=3, shift=0, wasted=7), R.sub("verbatim", wasted=7)])
    # bit depths and channel counts
    for bits in (8, 12, 16, 20, 24, 32):
        add(f"bits_{bits}", _walk(rng, 2, 80, bits), 32000, bits, block=40, subs=[R.sub("fixed", order=2), R.sub("verbatim")], stereo=10 if bits < 32 else 8)
    add("bits_from_streaminfo", _walk(rng, 1, 64, 16), 32000, 16, block=32, subs=[R.sub("fixed", order=1)], size_form="info")
    for ch in (1, 2, 3, 8):
        add(f"channels_{ch}", _walk(rng, ch, 48, 16), 22050, 16, block=24, subs=[R.sub("fixed", order=c % 5) for c in range(ch)])
    # stereo modes, also mixed in one stream
    for code, name in ((8, "left_side"), (9, "side_right"), (10, "mid_side")):
        add(f"stereo_{name}", _walk(rng, 2, 96, 16), 44100, 16, block=48, subs=[R.sub("fixed", order=2), R.sub("lpc", coefs=[3, -3, 1], precision=3, shift=0)], stereo=code)
    add("stereo_mixed", _walk(rng, 2, 128, 16), 44100, 16, block=32, subs=[R.sub("fixed", order=1)] * 2, stereo=lambda i: (None, 8, 9, 10)[i])
    add("stereo_extremes", np.array([[32767, -32768, 32767, -32768] * 4, [-32768, 32767, 32767, -32768] * 4]), 44100, 16, block=16, stereo=10)
    # blocking, last frames, numbering
    add("variable_blocking", _walk(rng, 2, 16 + 192 + 100 + 17, 16), 48000, 16, blocks=[16, 192, 100, 17], variable=True, subs=[R.sub("fixed", order=1)] * 2, stereo=8)
    add("short_last_frame", _walk(rng, 1, 192 * 2 + 5, 16), 48000, 16, block=192, subs=[R.sub("fixed", order=2)])
    add("frames_130_of_16", _walk(rng, 1, 130 * 16, 16), 48000, 16, block=16, subs=[R.sub("fixed", order=1)])
    add("variable_number_seam", _walk(rng, 1, 150, 16), 48000, 16, blocks=[100, 30, 20], variable=True, subs=[R.sub("fixed", order=0)])
    # every block-size code form: the table codes, and the 8- and 16-bit explicit forms
    for b in sorted(R.BLOCK_CODES):
        n = b + 7 if b >= 2304 else 2 * b + 7
        add(f"block_code_{R.BLOCK_CODES[b]}_{b}", _walk(rng, 1, n, 16, step=20), 24000, 16, block=b, subs=[R.sub("fixed", order=1)])
    add("block_form_8bit", _walk(rng, 1, 2 * 100, 16), 24000, 16, block=100, block_form="8")
    add("block_form_8bit_of_a_table_size", _walk(rng, 1, 2 * 192, 16), 24000, 16, block=192, block_form="8", subs=[R.sub("fixed", order=1)])
    add("block_form_16bit", _walk(rng, 1, 2 * 300, 16), 24000, 16, block=300, block_form="16", subs=[R.sub("fixed", order=1)])
    # every rate code form
    for rate in sorted(R.RATE_CODES):
        add(f"rate_table_{rate}", _walk(rng, 1, 32, 16), rate, 16, block=16)
    add("rate_from_streaminfo", _walk(rng, 1, 32, 16), 11025, 16, block=16, rate_form="info")
    add("rate_khz", _walk(rng, 1, 32, 16), 48000, 16, block=16, rate_form="khz")
    add("rate_hz", _walk(rng, 1, 32, 16), 44100, 16, block=16, rate_form="hz")
    add("rate_dahz", _walk(rng, 1, 32, 16), 352800, 16, block=16, rate_form="dahz")
    # metadata in front of the frames
    seek = b"".join(int(v).to_bytes(8, "big") + int(v // 2).to_bytes(8, "big") + (32).to_bytes(2, "big") for v in (0, 32))
    add("padding_and_seektable", _walk(rng, 2, 64, 16), 24000, 16, block=32, subs=[R.sub("fixed", order=2)] * 2, stereo=9,
        extra_blocks=[(1, bytes(57)), (3, seek), (4, b"\x04\x00\x00\x00test\x00\x00\x00\x00")])
    add("unknown_total_and_no_md5", _walk(rng, 1, 64, 16), 24000, 16, block=32, total=0, md5=False, subs=[R.sub("fixed", order=2)])
    add("no_frames", np.zeros((1, 0)), 24000, 16, blocks=[])
    stream, x, sizes = full_size()
    out[FULL] = dict(stream=stream, x=x, rate=44100, bits=16, sizes=sizes, device=True)
    return out


def device_cases():
    return {k: v for k, v in cases().items() if v["device"]}


def _repair(data, sizes):
    """The CRC-8 (when the header still parses far enough to know its length) and the CRC-16 of every frame recomputed, so that a mutation
    inside a frame is met by the parser and not by the checksums."""
    from tts_indic_server_f5_amd import wave_codec as W
    data, at = bytearray(data), sizes[0]
    for size in sizes[1:]:
        if at + size > len(data) or size < 8:
            break
        f = data[at:at + size]
        extra = 0 if f[4] < 0x80 else 7 - (f[4] ^ 0xFF).bit_length() if f[4] < 0xFF else 0
        hlen = 5 + extra + {6: 1, 7: 2}.get(f[2] >> 4, 0) + {12: 1, 13: 2, 14: 2}.get(f[2] & 15, 0)
        if hlen + 3 <= size:
            f[hlen] = W.flac_crc8(bytes(f[:hlen]))
        f[-2:] = W.flac_crc16(bytes(f[:-2])).to_bytes(2, "big")
        data[at:at + size] = f
        at += size
    return bytes(data)


def mutants(count=2000, seed=99):
    """`count` damaged streams from the small device cases, a fixed seed: byte flips (half of them with the frames' checksums repaired, so
    the parser meets them), truncations, splices of two streams, and a length field forced to its maximum (a metadata block's length,
    STREAMINFO's total, its block sizes, a frame's 16-bit block size, a partition order, an escape width)."""
    rng = np.random.default_rng(seed)
    base = [(k, v) for k, v in cases().items() if v["device"] and len(v["stream"]) < 4000]
    out = []
    while len(out) < count:
        name, v = base[int(rng.integers(len(base)))]
        s, sizes = bytearray(v["stream"]), v["sizes"]
        kind = int(rng.integers(8))
        if kind < 4 and len(s) > sizes[0]:                      # flips, in the frames more often than in the metadata
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(sizes[0] if rng.random() < 0.8 else 4, len(s)))
                s[at] = (s[at] ^ (1 << int(rng.integers(8)))) if rng.random() < 0.7 else int(rng.integers(256))
            m = _repair(s, sizes) if kind < 2 else bytes(s)
        elif kind == 4:
            m = bytes(s[:int(rng.integers(0, len(s)))])
        elif kind == 5:
            _, w = base[int(rng.integers(len(base)))]
            t = w["stream"]
            cut_a = int(np.cumsum(sizes)[int(rng.integers(len(sizes)))]) if rng.random() < 0.5 else int(rng.integers(len(s) + 1))
            cut_b = int(np.cumsum(w["sizes"])[int(rng.integers(len(w["sizes"])))]) if rng.random() < 0.5 else int(rng.integers(len(t) + 1))
            m = bytes(s[:cut_a]) + t[min(cut_b, len(t)):] if rng.random() < 0.5 else bytes(s[:cut_a]) + t[w["sizes"][0]:]
        else:
            which = int(rng.integers(6))
            if which == 0:
                s[5:8] = b"\xff\xff\xff"
            elif which == 1:
                s[21] |= 0x0F
                s[22:26] = b"\xff\xff\xff\xff"
            elif which == 2:
                s[8:12] = b"\xff\xff\xff\xff" if rng.random() < 0.5 else b"\x00\x00\xff\xff"
            elif len(s) > sizes[0] + 8:
                at = sizes[0]
                if which == 3:                                   # the first frame's block size, in the 16-bit form when it has that
                    s[at + 2] = 0x70 | (s[at + 2] & 15)
                    s[at + 5:at + 5] = b"\xff\xff"
                    sizes = [sizes[0], sizes[1] + 2] + sizes[2:]
                else:                                            # bytes early in the first subframe: partition order, escape width
                    j = at + 6 + int(rng.integers(1, 6))
                    if j < len(s):
                        s[j] = 0xFF if which == 4 else s[j] | 0x3F
            m = _repair(s, sizes)
        out.append(m)
    return out


def false_sync():
    """(stream, samples): a mono VERBATIM frame whose sample bytes spell a complete valid frame header -- sync, codes, number and its correct
    CRC-8 -- so the scan finds a frame start inside it that no chain may visit."""
    from tts_indic_server_f5_amd import wave_codec as W
    head = bytes([0xFF, 0xF8, 0x69, 0x08, 0x00, 15])             # block code 6 (8-bit form: 16 samples), 44.1 kHz, mono, 16 bits, frame 0
    head += bytes([W.flac_crc8(head)])
    assert W._flac_frame_header(head + bytes(9), 0, dict(rate=44100, bits=16))["block"] == 16
    spelled = np.frombuffer(head + b"\x00", dtype=">i2").astype(np.int64)
    x = np.concatenate([np.arange(5) * 100, spelled, np.arange(32 - 5 - len(spelled)) - 7])[None]
    stream, _ = R.write_flac(x, 44100, 16, block=16)
    assert stream.count(head) >= 1
    return stream, x


def refusals():
    """name -> a damaged stream that `read_flac` refuses, each for its own reason: the short list that also runs on the device, after
    tests/test_flac_in_core.py has run every one of them through the CPU build of the core."""
    from tts_indic_server_f5_amd import wave_codec as W
    c = cases()
    out = {}
    v = c["rice_14"]
    s = bytearray(v["stream"])
    s[v["sizes"][0] + 20] ^= 0x10
    out["a flipped bit in a Rice partition"] = bytes(s)
    s = bytearray(c["fixed_2"]["stream"])
    s[-1] ^= 0x01
    out["a flipped CRC-16 byte"] = bytes(s)
    out["a truncated last frame"] = c["stereo_mid_side"]["stream"][:-9]
    v = c["rice_0"]
    s = bytearray(v["stream"])
    s[len(s) - v["sizes"][-1] + 12:] = bytes(v["sizes"][-1] - 12)
    out["a unary run that reaches the stream's end"] = bytes(s)
    v = c["fixed_2"]
    s, at = bytearray(v["stream"]), v["sizes"][0]
    hlen = W._flac_frame_header(bytes(s), at, dict(rate=24000, bits=16))["size"]
    s[at + hlen + 1 + 4] |= 0x3C                                  # behind the subframe header and two warm-up samples: method, partition order
    out["a partition order too large for the block"] = _repair(s, v["sizes"])
    head = bytes([0xFF, 0xF8, 0x79, 0x08, 0x00, 0xFF, 0xFE])     # block code 7: 16-bit form, 65 535 samples
    frame = head + bytes([W.flac_crc8(head)]) + b"\x02" + bytes(7)
    frame += W.flac_crc16(frame).to_bytes(2, "big")
    s = R.stream_header(44100, 1, 16, 0) + frame
    assert len(s) == 60
    out["a header claiming 65 535 samples in a 60-byte stream"] = s
    return out
