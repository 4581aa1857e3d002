"""Waves in and out of the server, with nothing of the model in it: reading WAV files (`load_wav`), torchaudio's polyphase sinc resampler
(`rate_pair`, `resample_taps`, `resample_sinc_hann`) with its tap-table caches, the integer resampler of finished PCM (`resample_pcm16`,
`StreamResampler`), G.711 (`encode_g711`, `decode_g711`), the delivery format of a request (`delivery_format`, `deliver_pcm16`) and the bytes
of a response (`delivery_bytes`, `wav_bytes`, `wav_stream_header`).  A leaf module: `infer`, `serve` and `ops` import it, never the other way
round; `infer` and `serve` hand every public name on (`infer.load_wav`, `serve.wav_bytes`, ...)."""
from __future__ import annotations

import collections
import io
import math
import os
import struct
import threading
import wave as _wave

import numpy as np
import torch

LOWPASS_FILTER_WIDTH, ROLLOFF = 6, 0.99   # torchaudio.transforms.Resample's defaults, which the library builds in (csrc/rate_pair.h)
SAMPLE_RATE = 24000   # the model's rate (`infer.target_sample_rate`, which asserts that the two agree): what PCM is before delivery

MAX_TAP_TABLE_BYTES = 4 << 20   # resample_taps refuses larger tables (the largest supported pair, 11 025 -> 24 000 Hz, needs 206 KB)
TAP_TABLE_CACHE = 16             # rate pairs kept, on the host and per device: an upload chooses its rate, so neither cache may grow with it
_tap_tables: collections.OrderedDict = collections.OrderedDict()   # (orig_freq, new_freq, lowpass_filter_width, rolloff) -> resample_taps result


_tap_lock = threading.Lock()     # route handlers look tables up from a thread pool


def _lru_get(cache, key):
    with _tap_lock:
        hit = cache.get(key)
        if hit is not None:
            cache.move_to_end(key)
        return hit


def _lru_put(cache, key, value):
    with _tap_lock:
        cache[key] = value
        while len(cache) > TAP_TABLE_CACHE:
            cache.popitem(last=False)
        return value


def rate_pair(orig_freq: int, new_freq: int, lowpass_filter_width: int = LOWPASS_FILTER_WIDTH, rolloff: float = ROLLOFF):
    """(of, nf, width, L) of torchaudio.transforms.Resample(orig_freq, new_freq): of : nf the rate pair reduced by its gcd, width =
    ceil(lowpass_filter_width * of / (min(of, nf) * rolloff)) and L = 2 * width + of, the row length of the tap table.  Equal rates give
    (1, 1, 0, 0): no table, as in the library (csrc/rate_pair.h).  The one statement of the rule on the host."""
    orig, new = int(orig_freq), int(new_freq)
    if orig == new:
        return 1, 1, 0, 0
    g = math.gcd(orig, new)
    of, nf = orig // g, new // g
    width = math.ceil(lowpass_filter_width * of / (min(of, nf) * rolloff))
    return of, nf, width, 2 * width + of


def resample_taps(orig_freq: int, new_freq: int, lowpass_filter_width: int = LOWPASS_FILTER_WIDTH, rolloff: float = ROLLOFF):
    """The polyphase kernel of torchaudio.transforms.Resample(orig_freq, new_freq) ("sinc_interp_hann", torchaudio 2.6):
    (of, nf, width, taps fp32 [nf, 2 * width + of]) with of : nf the reduced rate pair -- computed in fp64, then cast to fp32.  Output
    j = q * nf + p of a clip is sum_k taps[p][k] * xpad[q * of + k], xpad = the clip with `width` zeros in front and `width + of` behind.
    The shape is `rate_pair`'s (equal rates, which nothing resamples: an empty [1, 0] table).
    Cached per rate pair, the `TAP_TABLE_CACHE` most recently used ones (treat the table as read-only).  A table above 4 MiB raises ValueError (e.g. 44 101 -> 24 000 Hz: several GB)."""
    key = (int(orig_freq), int(new_freq), lowpass_filter_width, rolloff)
    hit = _lru_get(_tap_tables, key)
    if hit is not None:
        return hit
    if key[0] < 1 or key[1] < 1:
        raise ValueError(f"sample rates must be positive (got {orig_freq} -> {new_freq})")
    of, nf, width, L = rate_pair(*key)
    base_freq = min(of, nf) * rolloff
    nbytes = 4 * nf * L
    if nbytes > MAX_TAP_TABLE_BYTES:
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz needs a {nf} x {L} tap table ({nbytes} bytes, limit {MAX_TAP_TABLE_BYTES}): "
                         "unsupported sample-rate pair")
    idx = torch.arange(-width, L - width, dtype=torch.float64)[None, None] / of
    t = torch.arange(0, -nf, -1, dtype=torch.float64)[:, None, None] / nf + idx
    t = (t * base_freq).clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base_freq / of)
    return _lru_put(_tap_tables, key, (of, nf, width, kernels.to(torch.float32)[:, 0].contiguous()))


def resample_sinc_hann(wave: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = LOWPASS_FILTER_WIDTH,
                       rolloff: float = ROLLOFF) -> torch.Tensor:
    """torchaudio.transforms.Resample(orig_freq, new_freq) (call site F/infer/utils_infer.py:430-432), default
    "sinc_interp_hann" method of torchaudio 2.6: polyphase windowed-sinc kernel (`resample_taps`) applied as a strided conv1d.
    wave [channels, n] -> [channels, ceil(n * new / orig)]."""
    if orig_freq == new_freq:
        return wave
    of, nf, width, taps = resample_taps(orig_freq, new_freq, lowpass_filter_width, rolloff)
    kernels = taps[:, None]
    shape = wave.shape
    w = wave.reshape(-1, shape[-1]).to(torch.float32)
    length = w.shape[-1]
    w = torch.nn.functional.pad(w, (width, width + of))
    out = torch.nn.functional.conv1d(w[:, None], kernels, stride=of)
    out = out.transpose(1, 2).reshape(w.shape[0], -1)
    target = math.ceil(nf * length / of)
    return out[..., :target].reshape(*shape[:-1], target)


def resampled_length(n: int, orig_freq: int, new_freq: int) -> int:
    """Samples `resample_sinc_hann` returns for n: ceil(nf * n / of), in integers (its math.ceil of the float quotient gives the same for
    every clip length in reach: an exact quotient is an exact float, and no other comes within an ulp of an integer below 2^52)."""
    of, nf, _, _ = rate_pair(orig_freq, new_freq)
    return -(-nf * int(n) // of)


_taps_on_device: collections.OrderedDict = collections.OrderedDict()   # (orig_freq, new_freq, device) -> the tap table there


def _device_taps(orig_freq, new_freq, device):
    key = (int(orig_freq), int(new_freq), str(device))
    hit = _lru_get(_taps_on_device, key)
    return hit if hit is not None else _lru_put(_taps_on_device, key, resample_taps(orig_freq, new_freq)[3].to(device))


_WAVE_FORMAT_PCM, _WAVE_FORMAT_IEEE_FLOAT, _WAVE_FORMAT_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
_KSDATAFORMAT_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"   # bytes 2..15 of every KSDATAFORMAT_SUBTYPE_* GUID
_WAVE_FORMAT_NAMES = {0x0002: "MS ADPCM", 0x0006: "A-law", 0x0007: "mu-law", 0x0011: "IMA ADPCM", 0x0031: "GSM 6.10",
                      0x0050: "MPEG", 0x0055: "MPEG Layer 3", 0x00FF: "AAC", 0x1610: "HE-AAC", 0xF1AC: "FLAC"}


def _wave_format_name(tag):
    return f"format code {tag:#06x}" + (f" ({_WAVE_FORMAT_NAMES[tag]})" if tag in _WAVE_FORMAT_NAMES else "")


def load_wav(src):
    """WAV file -> (float32 tensor [channels, samples], sample_rate), scaled like torchaudio.load: PCM 8-bit unsigned
    ((x - 128) / 128), 16/24/32-bit signed (/ 2**15, / 2**23, / 2**31), IEEE float 32/64-bit as stored; WAVE_FORMAT_EXTENSIBLE with a
    PCM or float sub-format; any channel count.  `src` is a path, the file's bytes, or a binary file object.  A small RIFF chunk walker
    instead of the stdlib `wave` module, which reads neither float nor EXTENSIBLE files.  Anything else (FLAC, MP3, compressed WAV
    format codes, a truncated file) raises ValueError naming what was found."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        data = bytes(src)
    elif hasattr(src, "read"):
        data = src.read()
    else:
        with open(os.fspath(src), "rb") as f:
            data = f.read()
    if data[:4] == b"fLaC":
        raise ValueError("not a WAV file: FLAC stream ('fLaC' magic)")
    if data[:3] == b"ID3" or (len(data) > 1 and data[0] == 0xFF and data[1] & 0xE0 == 0xE0):
        raise ValueError("not a WAV file: MPEG audio (MP3) stream")
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"not a RIFF/WAVE file (starts with {data[:12]!r})")
    fmt = body = None
    pos = 12
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        start, end = pos + 8, pos + 8 + size
        if cid == b"fmt ":
            if end > len(data) or size < 16:
                raise ValueError(f"truncated WAV: 'fmt ' chunk of {size} bytes, {len(data) - start} present")
            fmt = data[start:end]
        elif cid == b"data":
            if end > len(data):
                raise ValueError(f"truncated WAV: 'data' chunk declares {size} bytes, {len(data) - start} present")
            body = data[start:end]
            if fmt is not None:
                break
        pos = end + (size & 1)          # chunks are word-aligned
    if fmt is None or body is None:
        raise ValueError("truncated WAV: no " + ("'fmt '" if fmt is None else "'data'") + " chunk")
    tag, ch, sr, _, _, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == _WAVE_FORMAT_EXTENSIBLE:
        if len(fmt) < 40:
            raise ValueError(f"truncated WAV: WAVE_FORMAT_EXTENSIBLE 'fmt ' chunk of {len(fmt)} bytes (needs 40)")
        guid = fmt[24:40]
        sub = struct.unpack_from("<H", guid, 0)[0]
        if guid[2:] != _KSDATAFORMAT_TAIL:
            raise ValueError(f"unsupported WAV: WAVE_FORMAT_EXTENSIBLE with sub-format GUID {guid.hex()}")
        if sub not in (_WAVE_FORMAT_PCM, _WAVE_FORMAT_IEEE_FLOAT):
            raise ValueError(f"unsupported WAV: WAVE_FORMAT_EXTENSIBLE with sub-format {_wave_format_name(sub)}")
        tag = sub
    if ch < 1:
        raise ValueError(f"unsupported WAV: {ch} channels")
    if tag == _WAVE_FORMAT_PCM and bits in (8, 16, 24, 32):
        kind = "pcm"
    elif tag == _WAVE_FORMAT_IEEE_FLOAT and bits in (32, 64):
        kind = "float"
    elif tag in (_WAVE_FORMAT_PCM, _WAVE_FORMAT_IEEE_FLOAT):
        raise ValueError(f"unsupported WAV: {'PCM' if tag == _WAVE_FORMAT_PCM else 'IEEE float'} at {bits} bits per sample")
    else:
        raise ValueError(f"unsupported WAV: {_wave_format_name(tag)}")
    width = bits // 8
    n = len(body) // (width * ch)       # whole frames only, like wave.readframes
    raw = body[:n * width * ch]
    if kind == "float":
        x = np.frombuffer(raw, dtype="<f4" if bits == 32 else "<f8").astype(np.float32)
    elif bits == 8:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif bits == 16:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif bits == 24:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = ((v << 8) >> 8).astype(np.float32) / 8388608.0      # sign-extend the 24-bit value
    else:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    a = x.reshape(-1, ch).T
    return torch.from_numpy(np.ascontiguousarray(a)), sr


def quantise_pcm16(wave) -> np.ndarray:
    """int16 PCM of float samples by the routes' rule (`wav_bytes`, `pcm16`): rint(x * 32768) in float64, half to even, clipped."""
    return np.clip(np.rint(np.asarray(wave).astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


# ----------------------------------------- delivery format: output sample rate and G.711 (not in the reference, whose route always answers 24 kHz PCM)
OUTPUT_SAMPLE_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
OUTPUT_ENCODINGS = ("pcm16", "mulaw", "alaw")     # their position is the library's encoding code (include/f5hip.h f5hip_wave_encode)


def _polyphase_pcm(xpad, taps64, of, nq):
    """Polyphase blocks 0 .. nq - 1 over xpad (float64, at least nq * of + L - of samples): out[q * nf + p] = sum_k taps64[p][k] * xpad[q * of + k],
    k ascending, each product and each sum rounded to fp64 on its own; then rint (half to even), clipped, as int16."""
    nf, L = taps64.shape
    acc = np.zeros((nq, nf), dtype=np.float64)
    for k in range(L):
        acc += xpad[k:k + (nq - 1) * of + 1:of, None] * taps64[None, :, k]
    return np.clip(np.rint(acc), -32768, 32767).astype(np.int16).reshape(-1)


def _output_taps(new_freq):
    of, nf, width, taps = resample_taps(SAMPLE_RATE, delivery_format(new_freq)[0])
    return of, nf, width, taps.numpy().astype(np.float64)


def _as_pcm16(pcm):
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise ValueError(f"expected 1-D int16 PCM (got {pcm.dtype}, {pcm.ndim}-D)")
    return pcm


def resample_pcm16(pcm, new_freq) -> np.ndarray:
    """24 kHz int16 PCM [n] at `new_freq` (one of OUTPUT_SAMPLE_RATES): int16 [resampled_length(n, 24000, new_freq)].  Output j = q nf + p is
    rint(sum_k (double)taps[p][k] * (double)xpad[q of + k]) -- `resample_taps`' fp32 table, k ascending, fp64 accumulation, xpad = the samples
    with `width` zeros in front and zeros behind -- half to even, clipped to [-32768, 32767].  Integer samples times fp32 taps are exact in
    fp64 (16 + 24 bits), so a fused multiply-add and numpy's multiply-then-add give the same bits: the device kernel (csrc/wave_out.h
    wave_encode_kernel) is held to this function with no tolerance.  24000 returns its input."""
    pcm = _as_pcm16(pcm)
    if int(new_freq) == SAMPLE_RATE:
        return pcm
    of, nf, width, taps64 = _output_taps(new_freq)
    m = resampled_length(len(pcm), SAMPLE_RATE, new_freq)
    if m == 0:
        return np.zeros(0, dtype=np.int16)
    nq = -(-m // nf)
    xpad = np.zeros(nq * of + 2 * width, dtype=np.float64)
    xpad[width:width + len(pcm)] = pcm
    return _polyphase_pcm(xpad, taps64, of, nq)[:m]


class StreamResampler:
    """`resample_pcm16` one piece at a time: `feed(piece)` returns the outputs of every polyphase block whose input window is complete and keeps
    the tail it still needs, `flush()` the rest (zeros behind the last sample).  The concatenation of everything returned equals
    `resample_pcm16` of the concatenated input, bit for bit, whatever the piece sizes: an output's terms and their order do not depend on
    when it is computed."""

    def __init__(self, new_freq):
        self.new_freq = int(new_freq)
        self.identity = self.new_freq == SAMPLE_RATE
        if not self.identity:
            self.of, self.nf, self.width, self.taps64 = _output_taps(new_freq)
            self.tail = np.zeros(self.width, dtype=np.float64)   # xpad from block `q` on: the zeros in front at first
        self.n = self.q = 0                                      # samples fed; polyphase blocks emitted

    def feed(self, piece):
        piece = _as_pcm16(piece)
        if self.identity:
            return piece
        self.n += len(piece)
        self.tail = np.concatenate([self.tail, piece.astype(np.float64)])
        ready = max((self.n - self.width) // self.of, 0)         # block q needs xpad[q of .. q of + 2 width + of): width + n of it exist
        if ready <= self.q:
            return np.zeros(0, dtype=np.int16)
        out = _polyphase_pcm(self.tail, self.taps64, self.of, ready - self.q)
        self.tail = self.tail[(ready - self.q) * self.of:]
        self.q = ready
        return out

    def flush(self):
        if self.identity:
            return np.zeros(0, dtype=np.int16)
        m = resampled_length(self.n, SAMPLE_RATE, self.new_freq)
        nq = -(-m // self.nf) - self.q
        if nq <= 0:
            return np.zeros(0, dtype=np.int16)
        xpad = np.zeros(nq * self.of + 2 * self.width, dtype=np.float64)
        xpad[:len(self.tail)] = self.tail
        out = _polyphase_pcm(xpad, self.taps64, self.of, nq)[:m - self.q * self.nf]
        self.q, self.tail = self.q + nq, np.zeros(0, dtype=np.float64)
        return out


def _check_law(law):
    if law not in ("mulaw", "alaw"):
        raise ValueError(f'law must be "mulaw" or "alaw" (got {law!r})')


def encode_g711(pcm, law) -> np.ndarray:
    """G.711 code bytes (uint8) of int16 PCM: CPython's `audioop.lin2ulaw` / `lin2alaw` at width 2, in closed form.  mu-law works on the 14-bit
    value s >> 2 (magnitude clipped at 8158, bias 0x21), A-law on the 13-bit value s >> 3 (a negative value as -x - 1); the segment is the
    position of the leading bit."""
    _check_law(law)
    s = np.asarray(pcm)
    if s.dtype != np.int16:
        raise ValueError(f"expected int16 PCM (got {s.dtype})")
    ilog2 = lambda m: np.frexp(m.astype(np.float64))[1] - 1   # noqa: E731  floor(log2 m), m >= 1
    if law == "mulaw":
        x = s.astype(np.int32) >> 2
        sign = np.where(x < 0, 0x7F, 0xFF)
        m = np.minimum(np.abs(x), 8158) + 0x21
        seg = ilog2(m) - 5
        code = ((seg << 4) | ((m >> (seg + 1)) & 15)) ^ sign
    else:
        x = s.astype(np.int32) >> 3
        mask = np.where(x >= 0, 0xD5, 0x55)
        m = np.where(x >= 0, x, -x - 1)
        seg = np.maximum(ilog2(np.maximum(m, 1)) - 4, 0)
        code = ((seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 15)) ^ mask
    return code.astype(np.uint8)


def decode_g711(codes, law) -> np.ndarray:
    """int16 PCM of G.711 code bytes: `audioop.ulaw2lin` / `alaw2lin` at width 2."""
    _check_law(law)
    c = np.asarray(codes)
    if c.dtype != np.uint8:
        raise ValueError(f"expected uint8 codes (got {c.dtype})")
    c = c.astype(np.int32)
    if law == "mulaw":
        u = ~c & 0xFF
        t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
        out = np.where(u & 0x80, 0x84 - t, t - 0x84)
    else:
        a = c ^ 0x55
        seg = (a & 0x70) >> 4
        t = (a & 0x0F) << 4
        t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
        out = np.where(a & 0x80, t, -t)
    return out.astype(np.int16)


def delivery_format(sample_rate=None, encoding=None):
    """(rate, encoding) of a request with None filled in (24000, "pcm16"), checked against OUTPUT_SAMPLE_RATES / OUTPUT_ENCODINGS."""
    rate = SAMPLE_RATE if sample_rate is None else sample_rate
    enc = "pcm16" if encoding is None else encoding
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or int(rate) not in OUTPUT_SAMPLE_RATES:
        raise ValueError(f"sample_rate must be one of {list(OUTPUT_SAMPLE_RATES)} (got {sample_rate!r})")
    if not isinstance(enc, str) or enc not in OUTPUT_ENCODINGS:
        raise ValueError(f"encoding must be one of {list(OUTPUT_ENCODINGS)} (got {encoding!r})")
    return int(rate), enc


def deliver_pcm16(pcm, sample_rate=None, encoding=None) -> np.ndarray:
    """The delivery format of a request's canonical result, its 24 kHz int16 PCM: `resample_pcm16`, then `encode_g711` -- int16 at
    `sample_rate`, or uint8 code bytes.  (24000, "pcm16") returns the PCM itself."""
    rate, enc = delivery_format(sample_rate, encoding)
    pcm = resample_pcm16(pcm, rate)
    return pcm if enc == "pcm16" else encode_g711(pcm, enc)


_G711_TAGS = {"mulaw": 7, "alaw": 6}   # WAVE_FORMAT_MULAW, WAVE_FORMAT_ALAW


def _g711_header(encoding, sample_rate, n, riff_size, data_size):
    """RIFF header of a mono G.711 WAV: an 18-byte `fmt ` chunk (format tag 7 / 6, 8 bits per sample, block align 1, byte rate = sample rate,
    cbSize 0), a `fact` chunk with the sample count, and the `data` chunk's header."""
    return (b"RIFF" + struct.pack("<I", riff_size) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHHH", 18, _G711_TAGS[encoding], 1, sample_rate, sample_rate, 1, 8, 0)
            + b"fact" + struct.pack("<II", 4, n) + b"data" + struct.pack("<I", data_size))


def delivery_bytes(audio, encoding: str = "pcm16") -> bytes:
    """The body bytes of samples in any of the forms a request's result takes: uint8 G.711 codes as they are, int16 PCM little-endian, float
    samples by `pcm16`'s rule -- and, for a G.711 `encoding`, PCM that is not encoded yet through `encode_g711`."""
    a = np.asarray(audio)
    if a.dtype == np.uint8:
        return a.tobytes()
    if a.dtype != np.int16:
        a = quantise_pcm16(a)
    if encoding != "pcm16":
        return encode_g711(a, encoding).tobytes()
    return a.astype("<i2").tobytes()


def wav_bytes(audio: np.ndarray, sample_rate: int = SAMPLE_RATE, encoding: str = "pcm16") -> io.BytesIO:
    """A mono WAV file of `audio` (`delivery_bytes`) at `sample_rate`: 16-bit PCM, or G.711 (`_g711_header`) for "mulaw" / "alaw"."""
    if encoding not in OUTPUT_ENCODINGS:
        raise ValueError(f"encoding must be one of {list(OUTPUT_ENCODINGS)} (got {encoding!r})")
    body = delivery_bytes(audio, encoding)
    buf = io.BytesIO()
    if encoding == "pcm16":
        with _wave.open(buf, "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(sample_rate)
            f.writeframes(body)
    else:
        pad = len(body) & 1                      # chunks are word-aligned
        buf.write(_g711_header(encoding, sample_rate, len(body), 4 + 26 + 12 + 8 + len(body) + pad, len(body)) + body + b"\x00" * pad)
    buf.seek(0)
    return buf


def pcm16(audio: np.ndarray) -> bytes:
    """Little-endian int16 PCM bytes of float samples, by `wav_bytes`'s rule: rint(x * 32768), clipped."""
    return quantise_pcm16(audio).astype("<i2").tobytes()


def wav_stream_header(sample_rate: int = SAMPLE_RATE, encoding: str = "pcm16") -> bytes:
    """Header of a mono WAV of unknown length: RIFF and `data` sizes are 0xFFFFFFFF (the usual streaming-WAV convention; players read to the
    end of the stream).  16-bit PCM: 44 bytes; G.711: 58 bytes, the `fact` chunk's sample count 0xFFFFFFFF too."""
    if encoding != "pcm16":
        return _g711_header(encoding, sample_rate, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    return (b"RIFF" + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, sample_rate, sample_rate * 2, 2, 16)
            + b"data" + struct.pack("<I", 0xFFFFFFFF))
