"""Waves in and out of the server, with nothing of the model in it: reading WAV files (`load_wav`), torchaudio's polyphase sinc resampler
(`rate_pair`, `resample_taps`, `resample_sinc_hann`) with its tap-table caches, the integer resampler of finished PCM (`resample_pcm16`,
`StreamResampler`), the BS.1770 loudness meter and normaliser (`measure_loudness`, `normalise_loudness_pcm16`), G.711 (`encode_g711`,
`decode_g711`), FLAC (`encode_flac`, `decode_flac`, `StreamFlacEncoder`; the whole format in: `read_flac`, `load_audio`), the delivery
format of a request (`delivery_format`, `deliver_pcm16`), time-scale modification of finished PCM (`wsola_pcm16`, `shift_pcm16`: a request's
`tempo` and `pitch`; `psola_pcm16`: a `pitch` that keeps the formants, a request's `keep_formants`), the provenance watermark (`mark_pcm16`, `detect_watermark`: a request's `watermark` key), all nine of these options -- five of delivery, two of prosody, the key and the flag -- as one value (`WaveSpec`, `WAVE_OPTIONS`; `StreamDelivery` applies it to a stream) and the bytes of a response (`delivery_bytes`, `wav_bytes`, `wav_stream_header`).  A leaf module: `infer`, `serve` and `ops` import it, never the other way
round; `infer` and `serve` hand every public name on (`infer.load_wav`, `serve.wav_bytes`, ...)."""
from __future__ import annotations

import collections
import dataclasses
import hashlib
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
FLAC_ENCODINGS = ("flac",)                        # beside them, not among them: a FLAC result is a whole stream (`encode_flac`), not samples
ALL_ENCODINGS = OUTPUT_ENCODINGS + FLAC_ENCODINGS


def _polyphase_pcm(xpad, taps64, of, nq):
    """Polyphase blocks 0 .. nq - 1 over xpad (float64, at least nq * of + L - of samples): out[q * nf + p] = sum_k taps64[p][k] * xpad[q * of + k],
    k ascending, each product and each sum rounded to fp64 on its own; then rint (half to even), clipped, as int16."""
    nf, L = taps64.shape
    acc = np.zeros((nq, nf), dtype=np.float64)
    for k in range(L):
        acc += xpad[k:k + (nq - 1) * of + 1:of, None] * taps64[None, :, k]
    return np.clip(np.rint(acc), -32768, 32767).astype(np.int16).reshape(-1)


def _polyphase_whole(pcm, of, nf, width, taps64):
    """A whole int16 wave through `_polyphase_pcm`: ceil(nf n / of) outputs, `width` zeros in front of the samples and zeros behind."""
    m = -(-nf * len(pcm) // of)
    if m == 0:
        return np.zeros(0, dtype=np.int16)
    nq = -(-m // nf)
    xpad = np.zeros(nq * of + 2 * width, dtype=np.float64)
    xpad[width:width + len(pcm)] = pcm
    return _polyphase_pcm(xpad, taps64, of, nq)[:m]


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
    return _polyphase_whole(pcm, *_output_taps(new_freq))


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
    """(rate, encoding) of a request with None filled in (24000, "pcm16"), checked against OUTPUT_SAMPLE_RATES and OUTPUT_ENCODINGS +
    FLAC_ENCODINGS."""
    rate = SAMPLE_RATE if sample_rate is None else sample_rate
    enc = "pcm16" if encoding is None else encoding
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or int(rate) not in OUTPUT_SAMPLE_RATES:
        raise ValueError(f"sample_rate must be one of {list(OUTPUT_SAMPLE_RATES)} (got {sample_rate!r})")
    if not isinstance(enc, str) or enc not in ALL_ENCODINGS:
        raise ValueError(f"encoding must be one of {list(ALL_ENCODINGS)} (got {encoding!r})")
    return int(rate), enc


def deliver_pcm16(pcm, sample_rate=None, encoding=None, flac_level=None) -> np.ndarray:
    """The delivery format of a request's canonical result, its 24 kHz int16 PCM: `resample_pcm16`, then `encode_g711` or `encode_flac` --
    int16 at `sample_rate`, uint8 code bytes, or a uint8 array that holds the FLAC stream (at `flac_level`, which only a FLAC request may
    name).  (24000, "pcm16") returns the PCM itself."""
    rate, enc = delivery_format(sample_rate, encoding)
    level = request_flac_level(flac_level, enc)
    pcm = resample_pcm16(pcm, rate)
    if enc in FLAC_ENCODINGS:
        return encode_flac(pcm, rate, level)
    return pcm if enc == "pcm16" else encode_g711(pcm, enc)


DELIVERY_OPTIONS = ("remove_silence", "loudness", "sample_rate", "encoding", "flac_level")
PROSODY_OPTIONS = ("tempo", "pitch")              # beside them: time-scale modification of the finished PCM (`shift_pcm16`)
WHOLE_WAVE = ("remove_silence, sample_rate and encoding need the request's whole wave: they are not available for a list of chunk texts (a streamed "
              "request, whose owner applies the delivery format piece by piece: StreamResampler, encode_g711) or with join=False")
WHOLE_WAVE_LOUDNESS = ("loudness is measured on the request's whole wave: it is not available for a list of chunk texts, on a streaming path or "
                       "with join=False")
WHOLE_WAVE_PROSODY = ("tempo and pitch are applied to the request's whole wave: they are not available for a list of chunk texts, on a streaming "
                      "path or with join=False")


@dataclasses.dataclass(frozen=True)
class WaveSpec:
    """What a request asks of its finished wave, the five `DELIVERY_OPTIONS`, the two `PROSODY_OPTIONS`, its `watermark` and its
    `keep_formants` flag (`WAVE_OPTIONS`) as one immutable, hashable value: the planner makes it (`WaveSpec.of`), and every finishing path -- `infer.finish_pcm16` on the host, `infer._finish_on_device`,
    `StreamDelivery` for a stream -- reads it.
    All are pure functions of the request's canonical result, its joined 24 kHz wave quantised to int16 PCM, applied in this order:
      `remove_silence`  the reference's `remove_silence_for_generated_wav` (`audio_prep.remove_silence_pcm`): pauses of 1 s or more shrink
                        to 500 ms on each side; the result is int16 PCM whatever the caller wanted otherwise.
      `tempo`, `pitch`  time-scale modification (`shift_pcm16`: WSOLA, then a rational resampler for the pitch): the duration divided by
                        `tempo` (0.5 to 2 in steps of 0.01) at the same pitch, the pitch moved by `pitch` whole semitones (-6 to 6) at the
                        same duration; 1.0 and 0 keep the samples as they are.  So loudness is measured on what is delivered.
      `keep_formants`   beside a non-zero `pitch` only (`check_keep_formants`): the pitch moves by `psola_pcm16` and the spectral envelope
                        stays; WSOLA then stretches by the tempo alone (`stretch`).
      `watermark`       a key, or a `WatermarkTag(key, id)` with a trace id (`check_watermark`): `mark_pcm16` behind the prosody step and in
                        front of the loudness step, so the level and the -1 dBFS peak cap are measured on the marked samples; None: no mark.
      `loudness`        a programme loudness target in LUFS within LOUDNESS_RANGE (ITU-R BS.1770-4; `normalise_loudness_pcm16`: the sample
                        peak stays at or below -1 dBFS); None keeps the level as synthesized.
      `sample_rate`, `encoding`  the delivery format (`deliver_pcm16`): one of OUTPUT_SAMPLE_RATES (`resample_pcm16`), then "pcm16", "mulaw" /
                        "alaw" (`encode_g711`: uint8 code bytes) or "flac" (`encode_flac`: a uint8 array that holds the whole stream).
      `flac_level`      0, or 1 for LPC subframes among the candidates of the stream's full blocks (never larger, the same samples); only a
                        "flac" request may name one: beside any other encoding a level is refused, never ignored.
    `remove_silence`, `loudness`, `tempo`, `pitch`, `watermark`, and a format other than 24 kHz "pcm16", need the request's whole wave
    (`needs_whole_wave`): they are refused for a list of chunk texts and with join=False; a stream applies the format piece by piece and
    refuses the others."""
    remove_silence: bool = False
    loudness: float | None = None
    sample_rate: int = SAMPLE_RATE
    encoding: str = "pcm16"
    flac_level: int = 0
    tempo: float = 1.0
    pitch: int = 0
    watermark: int | WatermarkTag | None = None
    keep_formants: bool = False

    @classmethod
    def of(cls, options) -> "WaveSpec":
        """The spec of a mapping of options: a missing key or None is the default, other keys are ignored.  The one place where they are
        checked together -- `check_loudness`, `request_flac_level`, `delivery_format`, then `check_tempo`, `check_pitch`,
        `prosody_stretch`, `check_watermark` and `check_keep_formants`, in that order, with their messages (ValueError).  A `watermark` of
        `{"id": I}` alone is refused here: only a service knows a key of its own (`serve.check_request_options` resolves it first)."""
        get = options.get
        loudness = check_loudness(get("loudness"))
        level = request_flac_level(get("flac_level"), get("encoding"))
        fmt = delivery_format(get("sample_rate"), get("encoding"))
        hundredths, pitch = check_tempo(get("tempo")), check_pitch(get("pitch"))
        prosody_stretch(hundredths, pitch)
        return cls(bool(get("remove_silence")), loudness, *fmt, level, hundredths / 100, pitch, check_watermark(get("watermark")),
                   check_keep_formants(get("keep_formants"), pitch))

    @property
    def format(self):
        return self.sample_rate, self.encoding

    @property
    def plain_format(self) -> bool:
        return self.format == (SAMPLE_RATE, "pcm16")

    @property
    def flac(self) -> bool:
        return self.encoding in FLAC_ENCODINGS

    @property
    def gain_constant(self):
        """`loudness_gain_constant` of the target, what `ops.wave_loudness` takes; None without one."""
        return None if self.loudness is None else loudness_gain_constant(self.loudness)

    @property
    def prosody(self) -> bool:
        """Whether `tempo` or `pitch` changes the samples."""
        return self.tempo != 1.0 or self.pitch != 0

    @property
    def stretch(self):
        """(P, Q) of the WSOLA step, what `ops.wave_prosody` takes beside the pitch; with `keep_formants` the tempo's alone."""
        hundredths = check_tempo(self.tempo)
        return formant_stretch(hundredths) if self.keep_formants else prosody_stretch(hundredths, self.pitch)

    def needs_whole_wave(self, streamed=False) -> bool:
        """Whether the request cannot be handed out chunk by chunk.  `streamed`: the format does not count, the stream's owner applies it."""
        return self.remove_silence or self.loudness is not None or self.prosody or self.watermark is not None or not (streamed or self.plain_format)

    def whole_wave_message(self) -> str:
        """The refusal of a request that `needs_whole_wave` where it cannot have it: `WHOLE_WAVE_LOUDNESS` when `loudness` is the reason,
        `WHOLE_WAVE_PROSODY` when `tempo` / `pitch` are the only one, `WHOLE_WAVE_WATERMARK` when the mark is."""
        if self.watermark is not None and not dataclasses.replace(self, watermark=None).needs_whole_wave():
            return WHOLE_WAVE_WATERMARK
        if self.prosody and not self.remove_silence and self.loudness is None and self.plain_format:
            return WHOLE_WAVE_PROSODY
        return WHOLE_WAVE_LOUDNESS if self.loudness is not None and not self.remove_silence else WHOLE_WAVE


WAVE_OPTIONS = tuple(f.name for f in dataclasses.fields(WaveSpec))   # DELIVERY_OPTIONS + PROSODY_OPTIONS + WATERMARK_OPTIONS + FORMANT_OPTIONS


# ----------------------------------------- loudness: the mono programme loudness of ITU-R BS.1770-4 on a request's 24 kHz int16 PCM, in integers
# up to one sqrt, so that the device meter (csrc/wave_out.h wave_kweight_kernel / wave_gate_kernel / wave_gain_kernel) is held to these
# functions bit for bit: no sum below depends on the order of its terms.
#   K-weighting  y[j] = sum_k h[k] x[j - k] (zeros in front), h = `loudness_taps()`: the impulse response of the two K-weighting biquads
#                designed for 24 kHz, LOUDNESS_TAPS = 1024 taps at 2^16, rounded; z[j] = y[j] >> 14 (floor)
#   sub-blocks   e[s] = sum of z^2 over the 2400 samples (100 ms) of sub-block s; only whole sub-blocks count
#   blocks       400 ms with 75 % overlap: E[b] = (e[b] + e[b+1] + e[b+2] + e[b+3]) >> 8, ns - 3 of them
#   gates        absolute E[b] > LOUDNESS_GATE_ABS (-70 LUFS); relative E[b] > floor(S1 / (10 n1)) (-10 LU) over the blocks that pass the
#                absolute one; n2, S2: count and sum of the blocks that pass both
#   scale        z is y / 2^14 = 2^2 x 32768 x (K-weighted sample at full scale 1), so a block's mean square is E 2^8 / (9600 2^34)
# Bit budget: sum |h| = 212 915 < 2^17.7, so |y| < 2^32.7 (exact in fp64 and in int64), |z| < 2^18.7, e < 2400 2^37.4 < 2^48.7,
# E < 2^42.7, and S below 2^62.5 for any request below 2^31 samples (fewer than 2^19.8 blocks).
LOUDNESS_TAPS = 1024
LOUDNESS_TAP_SHIFT, LOUDNESS_Y_SHIFT, LOUDNESS_E_SHIFT = 16, 14, 8
LOUDNESS_SUBBLOCK = 2400                               # 100 ms
LOUDNESS_BLOCK = 4 * LOUDNESS_SUBBLOCK                 # 400 ms
_LOUDNESS_SCALE = float(LOUDNESS_BLOCK) * 2.0 ** 26    # E of a block whose mean square is 1 (full scale): 9600 2^34 / 2^8
LOUDNESS_GATE_ABS = math.floor(10.0 ** ((-70.0 + 0.691) / 10.0) * _LOUDNESS_SCALE)
LOUDNESS_PEAK_CEILING = 29203                          # sample-peak ceiling of a normalised wave: -1 dBFS, floor(32767 * 10^(-1/20))
LOUDNESS_RANGE = (-40.0, -5.0)                         # targets a request may name, LUFS
_loudness_taps = None


def _kweight_biquads(fs):
    """(b, a) of the K-weighting shelf and high-pass for the rate fs, a[0] = 1: the analytic form libebur128 and pyloudnorm use (at
    48 kHz the table of BS.1770)."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = ([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0],
             [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    high = ([1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return shelf, high


def loudness_taps() -> np.ndarray:
    """The K-weighting filter as LOUDNESS_TAPS integer taps (int64, read-only): h[k] = rint(2^16 k_true[k]), k_true the impulse response of
    the two biquads of `_kweight_biquads(24000)`, run in fp64.  Computed once.  The taps from index 916 on round to zero."""
    global _loudness_taps
    if _loudness_taps is None:
        x = [1.0] + [0.0] * (LOUDNESS_TAPS - 1)
        for b, a in _kweight_biquads(float(SAMPLE_RATE)):
            y, x1, x2, y1, y2 = [], 0.0, 0.0, 0.0, 0.0
            for v in x:
                w = b[0] * v + b[1] * x1 + b[2] * x2 - a[1] * y1 - a[2] * y2
                x2, x1, y2, y1 = x1, v, y1, w
                y.append(w)
            x = y
        taps = np.rint(np.asarray(x, dtype=np.float64) * 2.0 ** LOUDNESS_TAP_SHIFT).astype(np.int64)
        # the bit budget every later step leans on: |y| <= sum|h| 32768 < 2^33 (exact in fp64), |z| = |y| >> 14 < 2^19
        assert (int(np.abs(taps).sum()) * 32768) >> LOUDNESS_Y_SHIFT < 1 << 19, int(np.abs(taps).sum())
        taps.setflags(write=False)
        _loudness_taps = taps
    return _loudness_taps


def measure_loudness(pcm):
    """(n2, S2, peak) of 24 kHz int16 PCM by the definition above, Python integers: the count and the sum of the gated 400 ms block
    energies E, and max |x|.  A wave shorter than 9600 samples has no block: n2 = 0."""
    pcm = _as_pcm16(pcm)
    n = len(pcm)
    peak = int(np.abs(pcm.astype(np.int32)).max()) if n else 0
    ns = n // LOUDNESS_SUBBLOCK
    if ns < 4:
        return 0, 0, peak
    h = np.trim_zeros(loudness_taps(), "b").astype(np.float64)
    # every product and every partial sum is an integer below 2^53 in magnitude: the fp64 convolution is exact in any order
    y = np.convolve(pcm[:ns * LOUDNESS_SUBBLOCK].astype(np.float64), h)[:ns * LOUDNESS_SUBBLOCK].astype(np.int64)
    z = y >> LOUDNESS_Y_SHIFT
    e = (z * z).reshape(ns, LOUDNESS_SUBBLOCK).sum(axis=1)
    E = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) >> LOUDNESS_E_SHIFT
    E = E[E > LOUDNESS_GATE_ABS]
    if not len(E):
        return 0, 0, peak
    S1 = sum(int(v) for v in E)
    E = E[E > S1 // (10 * len(E))]
    return len(E), sum(int(v) for v in E), peak


def loudness_lufs(n2, S2):
    """The loudness in LUFS of `measure_loudness`' (n2, S2): -0.691 + 10 log10 of the gated blocks' mean square; None when nothing passed
    the gates."""
    if not n2:
        return None
    return -0.691 + 10.0 * math.log10(S2 * 2.0 ** LOUDNESS_E_SHIFT / (n2 * float(LOUDNESS_BLOCK) * 2.0 ** 34))


def check_loudness(target):
    """A request's `loudness` option: None (absent), or a finite number of LUFS within LOUDNESS_RANGE, returned as float; a bool, any
    other type and a value outside the range are a ValueError."""
    if target is None:
        return None
    if isinstance(target, (bool, np.bool_)) or not isinstance(target, (int, float, np.integer, np.floating)):
        raise ValueError(f"loudness must be a number of LUFS (got {target!r})")
    target = float(target)
    if not math.isfinite(target) or not LOUDNESS_RANGE[0] <= target <= LOUDNESS_RANGE[1]:
        raise ValueError(f"loudness must be between {LOUDNESS_RANGE[0]:g} and {LOUDNESS_RANGE[1]:g} LUFS (got {target}).")
    return target


def loudness_gain_constant(target) -> float:
    """K_T of a target in LUFS: the E of a block at that loudness, 10^((target + 0.691) / 10) 9600 2^26 in fp64 -- what the device call
    takes per request (`ops.wave_loudness`)."""
    return 10.0 ** ((float(target) + 0.691) / 10.0) * _LOUDNESS_SCALE


def loudness_gain(n2, S2, peak, gain_k) -> float:
    """The gain that moves (n2, S2, peak) to K_T = `gain_k`: sqrt(K_T n2 / S2), at most LOUDNESS_PEAK_CEILING / peak; 1.0 when nothing
    passed the gates.  One correctly rounded fp64 operation per step: int -> fp64, *, /, sqrt, /, min."""
    if not n2:
        return 1.0
    return min(math.sqrt(gain_k * float(n2) / float(S2)), float(LOUDNESS_PEAK_CEILING) / float(peak))


def normalise_loudness_pcm16(pcm, target) -> np.ndarray:
    """24 kHz int16 PCM moved to `target` LUFS (`check_loudness`; None returns the input): out = clip(rint(x g)) in fp64, half to even, g =
    `loudness_gain` of `measure_loudness(pcm)` -- so the peak stays at or below LOUDNESS_PEAK_CEILING unless it was above before and the
    wave is quieter than the target.  A wave without a gated block (shorter than 400 ms, or silent) comes back unchanged.  What
    `ops.wave_loudness` equals byte for byte."""
    pcm, target = _as_pcm16(pcm), check_loudness(target)
    if target is None:
        return pcm
    n2, S2, peak = measure_loudness(pcm)
    if not n2:
        return pcm
    g = loudness_gain(n2, S2, peak, loudness_gain_constant(target))
    return np.clip(np.rint(pcm.astype(np.float64) * g), -32768, 32767).astype(np.int16)


# ----------------------------------------- prosody: a request's `tempo` and `pitch`, time-scale modification of its 24 kHz int16 PCM (WSOLA,
# then a rational resampler for the pitch) in integers with no freedom left -- so the device call (csrc/wave_out.h wave_wsola_kernel /
# wave_pitch_kernel, f5hip_wave_prosody) is held to `shift_pcm16` bit for bit, like every other back-end stage.
# `wsola_pcm16(x, P, Q)`: int16 x of length n -> int16 y of length m = ceil(n P / Q), the same pitch, 1/2 <= P / Q <= 2.
#   constants  PROSODY_FRAME L = 960 (40 ms), PROSODY_HOP H = 480, PROSODY_SEARCH D = 240 (10 ms)
#   window     W[i] = rint(32768 sin^2(pi (2 i + 1) / (2 L))) for i < H, in fp64, half to even; W[H + i] = 32768 - W[i]: two overlapping
#              frames weigh exactly 2^15 (csrc/wsola_window.inc holds the 480 integers; a test equates the two, so no libm decides a sample)
#   source     xt[j] = x[j] for 0 <= j < n, else 0
#   frames     K = ceil(m / H) + 1 of them; frame k's nominal start is p_k = floor(k H Q / P) - H (64-bit products); s_0 = -H
#   search     for k >= 1, with t = s_{k-1} + H (where frame k - 1 would go on): c(d) = sum_{i < L} |xt[p_k + d + i] - xt[t + i]|; d_k
#              minimises it over -D .. D, ties to the smaller |d|, then to the negative one; s_k = p_k + d_k
#   output     y[j] = (W[H + i] xt[s_k + H + i] + W[i] xt[s_{k+1} + i] + 16384) >> 15 (a floor shift), k = j // H, i = j - k H
# Bit budget: c < 960 * 65535 < 2^26 (a packed key c 2^9 + rank(d) below 2^35 orders cost, then the tie rule: rank(d) = 2 |d| - (d < 0));
# the numerator stays within 2^30 + 2^14; y is a convex combination up to rounding and never leaves int16: no clip.  P == Q gives the input
# back through the search (cost 0 at d = 0, which the tie rule prefers): `_wsola_frames` is the entry without the identity shortcut.
# Beyond a stretch of 2 the nominal starts advance by less than H / 2 = D and the search cannot reach the continuation of the frame before.
# `shift_pcm16(pcm, tempo, pitch)`: T = rint(100 tempo), p / q = PITCH_RATIOS[pitch]; the stretch P / Q = reduce(100 p, T q);
# `wsola_pcm16(pcm, P, Q)`, then for a pitch the polyphase arithmetic of `resample_pcm16` with the table `resample_taps(p, q)` (the pair
# plays the role of the rates): ceil(q m / p) samples, the duration n 100 / T and the pitch times p / q.
PROSODY_FRAME, PROSODY_HOP, PROSODY_SEARCH = 960, 480, 240
PROSODY_TEMPO_RANGE = (0.5, 2.0)
# p / q per semitone: within 2 cents of 2^(s / 12), each tap table (`rate_pair(p, q)`: q rows) below 11 KB; negative steps take the reciprocal
PITCH_RATIOS = {1: (18, 17), 2: (46, 41), 3: (44, 37), 4: (29, 23), 5: (4, 3), 6: (41, 29)}
PITCH_RATIOS.update({-s: (q, p) for s, (p, q) in list(PITCH_RATIOS.items())})
PITCH_RANGE = (-6, 6)
_wsola_window = None
_pitch_tables: dict = {}


def wsola_window() -> np.ndarray:
    """The WSOLA window, int64 [PROSODY_FRAME] (read-only): the rising half rounded from fp64, the falling half its complement to 2^15."""
    global _wsola_window
    if _wsola_window is None:
        i = np.arange(PROSODY_HOP, dtype=np.float64)
        rise = np.rint(32768.0 * np.sin(np.pi * (2.0 * i + 1.0) / (2.0 * PROSODY_FRAME)) ** 2).astype(np.int64)
        w = np.concatenate([rise, 32768 - rise])
        w.setflags(write=False)
        _wsola_window = w
    return _wsola_window


def check_tempo(tempo) -> int:
    """A request's `tempo` option as whole hundredths T: None (absent) is 100; a number from 0.5 to 2 whose hundredfold is a whole number
    (within 1e-9); a bool, any other type and any other value are a ValueError."""
    if tempo is None:
        return 100
    bad = ValueError(f"tempo must be a number from 0.5 to 2 in steps of 0.01 (got {tempo!r})")
    if isinstance(tempo, (bool, np.bool_)) or not isinstance(tempo, (int, float, np.integer, np.floating)):
        raise bad
    scaled = 100.0 * float(tempo)
    if not math.isfinite(scaled) or abs(scaled - round(scaled)) > 1e-9 or not 50 <= round(scaled) <= 200:
        raise bad
    return int(round(scaled))


def check_pitch(pitch) -> int:
    """A request's `pitch` option: None (absent) is 0; an int of whole semitones within PITCH_RANGE; a bool, a float and anything else are
    a ValueError."""
    if pitch is None:
        return 0
    if isinstance(pitch, (bool, np.bool_)) or not isinstance(pitch, (int, np.integer)) or not PITCH_RANGE[0] <= int(pitch) <= PITCH_RANGE[1]:
        raise ValueError(f"pitch must be a whole number of semitones from -6 to 6 (got {pitch!r})")
    return int(pitch)


def prosody_stretch(hundredths, pitch):
    """(P, Q) of a tempo in hundredths (`check_tempo`) and a pitch (`check_pitch`): the one WSOLA stretch reduce(100 p, T q) that both
    need; a stretch outside [1/2, 2] is a ValueError."""
    p, q = PITCH_RATIOS[pitch] if pitch else (1, 1)
    P, Q = 100 * p, int(hundredths) * q
    g = math.gcd(P, Q)
    P, Q = P // g, Q // g
    if P > 2 * Q or Q > 2 * P:
        raise ValueError(f"tempo {hundredths / 100} with pitch {pitch} stretches the wave by {P}/{Q}: outside 1/2 to 2")
    return P, Q


def wsola_rank(d):
    """The tie rank of a search offset: 0, -1, 1, -2, 2, ... -> 0, 1, 2, 3, 4, ..."""
    return 2 * np.abs(d) - (d < 0)


def _wsola_frames(x, P, Q):
    """(y int16 [ceil(n P / Q)], s: the frame starts s_0 .. s_{K-1}) of the definition above, with no shortcut for P == Q.  Per frame one
    [481, 960] table of absolute differences."""
    L, H, D = PROSODY_FRAME, PROSODY_HOP, PROSODY_SEARCH
    n = len(x)
    m = -(-n * P // Q)
    if m == 0:
        return np.zeros(0, dtype=np.int16), [-H]
    K = -(-m // H) + 1
    front = H + D                                                       # the least index read: p_1 - D >= -H - D
    back = ((K - 1) * H * Q) // P - H + D + L + H                       # an index no read reaches
    xt = np.zeros(front + max(back, n) + 1, dtype=np.int32)
    xt[front:front + n] = x
    rank = wsola_rank(np.arange(-D, D + 1, dtype=np.int64))
    s = [-H]
    for k in range(1, K):
        p = (k * H * Q) // P - H
        t = s[-1] + H
        cands = np.lib.stride_tricks.sliding_window_view(xt[front + p - D:front + p + D + L], L)
        cost = np.abs(cands - xt[front + t:front + t + L]).sum(axis=1, dtype=np.int64)
        s.append(p - D + int(np.argmin(cost * 512 + rank)))
    W = wsola_window()
    at = np.asarray(s, dtype=np.int64)[:, None] + np.arange(H, dtype=np.int64)[None] + front
    y = (W[H:] * xt[at[:-1] + H] + W[:H] * xt[at[1:]] + 16384) >> 15
    return y.reshape(-1)[:m].astype(np.int16), s


def wsola_pcm16(x, P, Q) -> np.ndarray:
    """int16 PCM x [n] stretched to ceil(n P / Q) samples at the same pitch, by the definition above; P == Q returns the input."""
    x = _as_pcm16(x)
    if isinstance(P, bool) or isinstance(Q, bool) or not all(isinstance(v, (int, np.integer)) for v in (P, Q)) or P < 1 or Q < 1:
        raise ValueError(f"wsola_pcm16: the stretch is a pair of positive ints (got {P!r}, {Q!r})")
    P, Q = int(P), int(Q)
    if P > 2 * Q or Q > 2 * P:
        raise ValueError(f"wsola_pcm16: a stretch of {P}/{Q} is outside 1/2 to 2")
    return x if P == Q else _wsola_frames(x, P, Q)[0]


def pitch_taps(pitch):
    """(of, nf, width, taps fp64 [nf, L]) of a pitch step: `resample_taps(p, q)` of its ratio, of = p, nf = q.  Computed once per step."""
    hit = _pitch_tables.get(pitch)
    if hit is None:
        of, nf, width, taps = resample_taps(*PITCH_RATIOS[pitch])
        hit = _pitch_tables[pitch] = (of, nf, width, taps.numpy().astype(np.float64))
    return hit


def shift_pcm16(pcm, tempo=None, pitch=None, keep_formants=False) -> np.ndarray:
    """A request's `tempo` and `pitch` on its 24 kHz int16 PCM [n], the host definition above: about n 100 / T samples, ceil(q ceil(n P /
    Q) / p) of them.  Both neutral (None, 1.0, 0) returns the input itself.  What `ops.wave_prosody` equals byte for byte.
    `keep_formants` (with a non-zero pitch; `check_keep_formants`): WSOLA by the tempo alone (`formant_stretch`), then `psola_pcm16`
    (defined below) in place of the extra stretch and the resampler: ceil(n 100 / T) samples.  The combined stretch is checked either way."""
    pcm = _as_pcm16(pcm)
    hundredths, pitch = check_tempo(tempo), check_pitch(pitch)
    keep = check_keep_formants(keep_formants, pitch)
    P, Q = prosody_stretch(hundredths, pitch)
    if hundredths == 100 and pitch == 0:
        return pcm
    if keep:
        return psola_pcm16(wsola_pcm16(pcm, *formant_stretch(hundredths)), pitch)
    y = wsola_pcm16(pcm, P, Q)
    return _polyphase_whole(y, *pitch_taps(pitch)) if pitch else y


def formant_stretch(hundredths):
    """(P, Q) of a tempo alone, reduce(100, T): the WSOLA stretch of a request that keeps its formants."""
    g = math.gcd(100, int(hundredths))
    return 100 // g, int(hundredths) // g


def shifted_length(n, stretch, pitch) -> int:
    """Samples `shift_pcm16` returns for n under `stretch` = (P, Q) and `pitch` (0 for a request that keeps its formants, with its
    `formant_stretch`)."""
    m = -(-int(n) * stretch[0] // stretch[1])
    if pitch:
        p, q = PITCH_RATIOS[pitch]
        m = -(-q * m // p)
    return m


# ----------------------------------------- formant-preserving pitch: a request's `keep_formants` beside a non-zero `pitch`.  Time-domain
# pitch-synchronous overlap-add (TD-PSOLA) on the 24 kHz int16 PCM, in integers with no freedom left, so the device call
# (csrc/wave_formant.h, f5hip_wave_prosody_formants; the rules are csrc/wave_formant_core.h) is held to `psola_pcm16` bit for bit.
# `psola_pcm16(x, pitch)`: int16 x [n] -> int16 y [n], the fundamental times p / q = PITCH_RATIOS[pitch], the spectral envelope kept.
#   source     xt[j] = x[j] for 0 <= j < n, else 0
#   track      frame f starts at t = 120 f (PSOLA_HOP), F = ceil(n / 120) frames.  d[l] = sum_{i < 480} |xt[t + i] - xt[t + l + i]| for the lags
#              l = 48 .. 400 (60 to 500 Hz), E = sum_{i < 480} |xt[t + i]|.  The lag: the smallest l with 8 d[l] <= 8 dmin + E, then upwards
#              while d[l + 1] < d[l] (l + 1 <= 400): the first dip within E / 8 of the best one, at its bottom.  ("The smallest lag within
#              25 % of dmin" locked onto 3 T on a 210 Hz vowel; a margin tied to the frame's level does not.)  Voiced iff E >= 64 * 480 and
#              2 d[lag] <= E.  d < 480 * 65535 < 2^25: exact integers.
#   marks      analysis marks (a, T, voiced) in one chain from t = 0, while t < n, the frame of t being t // 120:
#                unvoiced frame   a = t, T = 120
#                voiced frame     T = its lag.  After an unvoiced mark, or first: a = the position of the largest sample in [t, t + T).  After
#                                 a voiced mark: of the largest sample in [max(t - T // 8, a_prev + 24), t + T // 8].  Positions outside
#                                 the wave do not count; ties go to the earlier position.
#              then t = a + T.  The lower bound a_prev + 24 (half the smallest lag, never above t) makes every mark at least 24 samples
#              after the one before: at most ceil(n / 24) marks.
#   synthesis  u_0 = a_0, rem = 0; mark u takes the nearest analysis mark i (ties to the earlier one).  After a voiced i: u += (T_i q + rem)
#              // p, rem = (T_i q + rem) % p, so the mean spacing is exactly T q / p; after an unvoiced i: u += 120 and rem stays (noise is
#              not shifted).  While u < n.  A step is at least 48 * 29 // 41 = 33 samples.
#   window     w_T[k] = M[(|k| 1024) // T] for |k| <= T, M[j] = rint(32768 (1 + cos(pi j / 1024)) / 2), j = 0 .. 1024, in fp64, half to
#              even (csrc/psola_window.inc holds the 1025 integers; a test equates the two, so no libm decides a sample).  M[j] >= 1 up to
#              j = 1021, and (|k| 1024) // T <= 1021 for |k| < T <= 400: a grain weighs every sample inside it.
#   output     num[j] = sum over the synthesis marks (u, i) with |j - u| <= T_i of w_{T_i}[j - u] xt[a_i + j - u], den[j] the same sum of
#              the weights alone; y[j] = clip((2 num + den) // (2 den)) (a floor division: round half up) where den > 0, and y[j] = x[j]
#              where no grain covers j.  64-bit integers; no sum depends on an order.
# Consequences: len(y) == len(x); zeros stay zeros; a wave without a voiced frame comes back byte for byte (a_i = u_i = 120 i: every grain
# maps a sample onto itself, num = x den); nothing but the request's own samples enters.
PSOLA_HOP, PSOLA_WINDOW, PSOLA_LAG_MIN, PSOLA_LAG_MAX = 120, 480, 48, 400
PSOLA_MIN_ADVANCE = 24
PSOLA_TABLE = 1024
FORMANT_OPTIONS = ("keep_formants",)              # beside PROSODY_OPTIONS: the last `WaveSpec` field
_psola_window = None


def psola_window() -> np.ndarray:
    """The master Hann table M, int64 [PSOLA_TABLE + 1] (read-only): M[0] = 32768 down to M[1024] = 0."""
    global _psola_window
    if _psola_window is None:
        j = np.arange(PSOLA_TABLE + 1, dtype=np.float64)
        w = np.rint(32768.0 * (1.0 + np.cos(np.pi * j / PSOLA_TABLE)) / 2.0).astype(np.int64)
        w.setflags(write=False)
        _psola_window = w
    return _psola_window


def check_keep_formants(keep, pitch=None) -> bool:
    """A request's `keep_formants` option: None (absent) is False; a bool; anything else is a ValueError.  With `pitch` given (an int by
    `check_pitch`), True without a non-zero pitch is a ValueError too."""
    if keep is None:
        return False
    if not isinstance(keep, (bool, np.bool_)):
        raise ValueError(f"keep_formants must be true or false (got {keep!r})")
    if keep and pitch is not None and pitch == 0:
        raise ValueError("keep_formants needs a non-zero pitch")
    return bool(keep)


def psola_track(x):
    """(lag int64 [F], voiced bool [F]) of int16 x: the period track of the definition above, F = ceil(n / PSOLA_HOP)."""
    x = _as_pcm16(x)
    n, H, W, lo, hi = len(x), PSOLA_HOP, PSOLA_WINDOW, PSOLA_LAG_MIN, PSOLA_LAG_MAX
    F = -(-n // H)
    if F == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    N = (F - 1) * H + W
    xt = np.zeros(N + hi, dtype=np.int64)
    xt[:n] = x
    t = np.arange(F, dtype=np.int64) * H

    def frame_sums(e):
        cs = np.concatenate([[0], np.cumsum(e)])
        return cs[t + W] - cs[t]

    E = frame_sums(np.abs(xt[:N]))
    d = np.empty((F, hi - lo + 1), dtype=np.int64)
    for l in range(lo, hi + 1):
        d[:, l - lo] = frame_sums(np.abs(xt[:N] - xt[l:l + N]))
    first = np.argmax(8 * d <= (8 * d.min(axis=1) + E)[:, None], axis=1)
    lag = np.empty(F, dtype=np.int64)
    voiced = np.empty(F, dtype=bool)
    for f in range(F):
        row, l = d[f], int(first[f])
        while l + 1 < len(row) and row[l + 1] < row[l]:
            l += 1
        lag[f] = l + lo
        voiced[f] = E[f] >= 64 * W and 2 * row[l] <= E[f]
    return lag, voiced


def psola_marks(x, lag, voiced):
    """The analysis marks of int16 x under its track: int64 arrays (a, T, v), by the definition above."""
    x = _as_pcm16(x)
    n, a, T, v = len(x), [], [], []
    t, chained = 0, False
    while t < n:
        f = t // PSOLA_HOP
        if voiced[f]:
            L = int(lag[f])
            b, e = (max(t - L // 8, a[-1] + PSOLA_MIN_ADVANCE), t + L // 8 + 1) if chained else (t, t + L)
            e = min(e, n)
            at = b + int(np.argmax(x[b:e]))
            chained = True
        else:
            at, L, chained = t, PSOLA_HOP, False
        a.append(at); T.append(L); v.append(int(chained))
        t = at + L
    return np.asarray(a, dtype=np.int64), np.asarray(T, dtype=np.int64), np.asarray(v, dtype=np.int64)


def psola_synthesis(a, T, v, n, pitch):
    """The synthesis marks: int64 arrays (u, i), i the analysis mark each takes."""
    p, q = PITCH_RATIOS[pitch]
    us, idx = [], []
    if len(a):
        u, rem, i = int(a[0]), 0, 0
        while u < n:
            while i + 1 < len(a) and abs(int(a[i + 1]) - u) < abs(int(a[i]) - u):
                i += 1
            us.append(u); idx.append(i)
            if v[i]:
                step, rem = divmod(int(T[i]) * q + rem, p)
            else:
                step = int(T[i])
            u += step
    return np.asarray(us, dtype=np.int64), np.asarray(idx, dtype=np.int64)


def psola_pcm16(pcm, pitch) -> np.ndarray:
    """int16 PCM [n] with its fundamental moved by `pitch` semitones (1 .. 6 either way) and its formants kept, by the definition above:
    n samples.  What `ops.wave_prosody(..., keep_formants=...)` equals byte for byte."""
    x = _as_pcm16(pcm)
    pitch = check_pitch(pitch)
    if pitch == 0:
        raise ValueError("psola_pcm16: a non-zero pitch is needed")
    n = len(x)
    if n == 0:
        return x
    a, T, v = psola_marks(x, *psola_track(x))
    u, idx = psola_synthesis(a, T, v, n, pitch)
    M = psola_window()
    x64 = x.astype(np.int64)
    num, den = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for at, i in zip(u.tolist(), idx.tolist()):
        Ti, ai = int(T[i]), int(a[i])
        k = np.arange(max(-Ti, -at), min(Ti, n - 1 - at) + 1, dtype=np.int64)          # the grain's offsets whose output lies in the wave
        w = M[(np.abs(k) * PSOLA_TABLE) // Ti]
        src = ai + k
        inside = (src >= 0) & (src < n)
        num[at + k[0]:at + k[-1] + 1] += w * np.where(inside, x64[np.clip(src, 0, n - 1)], 0)
        den[at + k[0]:at + k[-1] + 1] += w
    covered = den > 0
    safe = np.where(covered, den, 1)
    y = np.where(covered, (2 * num + safe) // (2 * safe), x64)
    return np.clip(y, -32768, 32767).astype(np.int16)


# ----------------------------------------- provenance watermark: a request's `watermark` option (a key) adds a keyed, speech-shaped,
# spread-spectrum mark to its 24 kHz int16 PCM; `detect_watermark` scores a clip against keys.  The mark is integers only, so the device
# call (csrc/wave_mark.h, f5hip_wave_mark) is held to `mark_pcm16` bit for bit; the detector is floating point and scale-invariant.
#   constants  WATERMARK_PERIOD P = 16384 chips (0.68 s), WATERMARK_BLOCK = 240 (10 ms), WATERMARK_TAPS = 129, WATERMARK_SHIFT = 23,
#              WATERMARK_BAND = (22, 136): STFT bins of 1024 at 24 kHz, 516 to 3188 Hz
#   key        an int in 1 .. 2^48 - 1 (`check_watermark`)
#   chips      SplitMix64 with state `key`: state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;
#              z = (z ^ z >> 27) 0x94D049BB133111EB; z ^= z >> 31, all mod 2^64.  Bit i of output k is chip 64 k + i: +1 set, -1 clear
#   band taps  g[k] = rint(2^14 hann[k] (2 f1 sinc(2 f1 (k - 64)) - 2 f0 sinc(2 f0 (k - 64)))), f1 = 3200/24000, f0 = 500/24000, hann[k] =
#              0.5 - 0.5 cos(2 pi (k + 1) / 130), in fp64 (csrc/watermark_taps.inc holds the 129 integers; a test equates the two, so no
#              libm decides a sample); sum |g| = 34684
#   carrier    c[m] = (sum_k g[k] chip[(m - k + 64) mod P]) >> 3, a floor shift: |c| <= 4336 for any chips, int16
#   mark       A[b] = sum |x[j]| over block b (240 samples, the last one may be partial); E[b] = max(A[b-1], A[b], A[b+1]), a missing
#              neighbour counting 0; y[j] = clip(x[j] + ((E[j // 240] c[j mod P]) >> 23), -32768, 32767): 64-bit product, floor shift.
#              E <= 240 * 32768 = 2^23 * 0.9375, so |y - x| <= 4336 * 0.9375 = 4065 for any chips, and <= 4064 for every carrier whose
#              magnitude stays below 4335 (key 1: -2863 .. 3113); output block b depends on input blocks b-1 .. b+1 only
#   detect     frames of 1024 at hop 256 behind 768 zeros, window w[i] = sin(pi i / 1024), F = ceil((n + 768) / 256) frames, zeros behind
#              (`audio_prep.denoise_reference`'s framing); X = rfft(frame w); U[k] = X[k] / sqrt(|X[k]|^2 + 1e-10) inside the band, 0
#              outside; u = overlap-add of irfft(U) w, cropped to the clip; Z[m] = sum of u[j] over j = m mod P; r[o] = sum_m Z[m]
#              c[(m + o) mod P]; o* the smallest argmax; z = (r[o*] - mean r) / std r (population), 0 when std r = 0; detected = z >= 7.0.
#              Sample 0 of the clip was sample o* (mod P) of the marked wave.
# Threshold: r across offsets is close to Gaussian with about P 2.7 / 12 = 3700 independent values, so 7.0 gives about 5e-9 false alarms
# per (clip, key).
#
# Trace ids: a 30-bit payload beside the key (`WatermarkTag(key, id)`, `read_watermark`), carried as the rotation of three more carriers
# relative to the key's (code-shift keying).  Everything above stays; a key alone marks and scores as before.
#   constants  WATERMARK_ID_BITS = 30, WATERMARK_ID_SYMBOLS D = 3, WATERMARK_ID_STEP G = 16 (1024 rotations per symbol, 10 bits each),
#              WATERMARK_ID_MAX = 2^30 - 1, WATERMARK_ID_THRESHOLD = 6.0
#   sub-keys   `watermark_subkey(K, d)`, d = 0, 1, 2: 1 + (z mod (2^48 - 1)), z the SplitMix64 output number 257 + d of the generator
#              started at state K (outputs 1 .. 256 are the key's chips).  A sub-key is an ordinary key: its carrier c_d is
#              `watermark_carrier(subkey)`.  K = 1: 160832003273966, 194807364317806, 17338898203305
#   symbols    s_d = (id >> 10 d) & 1023
#   carrier    C[m] = 2 c_K[m] + sum_d c_d[(m - 16 s_d) mod P], int32, |C| <= 5 * 4336 = 21680
#   mark       A, E as above; y[j] = clip(x[j] + ((E[j // 240] C[j mod P]) >> 24), -32768, 32767): 64-bit product, floor shift.  Without an
#              id the sum over d is absent, and (2 c E) >> 24 == (c E) >> 23: a key alone is the mark above byte for byte.  E <= 2^23 *
#              0.9375, so |E C| / 2^24 <= 21680 * 0.9375 / 2 = 10162.5 and |y - x| <= 10163 (`WATERMARK_ID_DELTA_MAX`; the floor of a
#              negative half) for any chips.  The length is kept, zeros stay zeros, block b depends on blocks b-1 .. b+1 only
#   read       Z, the key's r_K, o* and z as above.  r_d = the correlation of Z with c_d by the same formula; candidate s takes
#              r_d[(o* - 16 s) mod P]; s_d = the smallest argmax over s = 0 .. 1023; z_d = (r_d there - mean r_d) / std r_d (population,
#              over all P offsets), 0 when std r_d = 0; id_z = min_d z_d.  The id (sum_d s_d << 10 d) is reported only when the key is
#              detected (z >= 7.0) and every z_d >= 6.0, otherwise None
# Threshold: the best of 1024 candidates at 6 sigma is about 1024 * 1e-9 = 1e-6 false symbols per symbol.
WATERMARK_PERIOD = 16384
WATERMARK_BLOCK = 240
WATERMARK_TAPS = 129
WATERMARK_SHIFT = 23
WATERMARK_BAND = (22, 136)
WATERMARK_THRESHOLD = 7.0
WATERMARK_MIN_SAMPLES = 12000
WATERMARK_MAX_SAMPLES = 1_440_000
WATERMARK_KEYS_MAX = 16
WATERMARK_KEY_MAX = (1 << 48) - 1
WATERMARK_OPTIONS = ("watermark",)                # beside DELIVERY_OPTIONS and PROSODY_OPTIONS: a `WaveSpec` field like them
WHOLE_WAVE_WATERMARK = ("watermark marks the request's whole wave: it is not available for a list of chunk texts, on a streaming path or "
                        "with join=False")
WATERMARK_ID_BITS = 30
WATERMARK_ID_SYMBOLS = 3
WATERMARK_ID_STEP = 16
WATERMARK_ID_MAX = (1 << WATERMARK_ID_BITS) - 1
WATERMARK_ID_THRESHOLD = 6.0
WATERMARK_ID_SHIFT = WATERMARK_SHIFT + 1           # the key's carrier counts twice in C
WATERMARK_ID_DELTA_MAX = 10163                     # |y - x| of a tagged request, for any chips
WATERMARK_ID_KEYS_MAX = 4                          # keys of one `ops.watermark_read_ids` call: four carrier rows each
_ID_SYMBOL_BITS = WATERMARK_ID_BITS // WATERMARK_ID_SYMBOLS
_ID_SYMBOL_COUNT = 1 << _ID_SYMBOL_BITS
WatermarkScore = collections.namedtuple("WatermarkScore", "key z offset detected")
WatermarkTag = collections.namedtuple("WatermarkTag", "key id")                    # a key and the trace id its mark carries
WatermarkRead = collections.namedtuple("WatermarkRead", "key z offset detected id id_z")
_watermark_taps = None
_watermark_carriers: collections.OrderedDict = collections.OrderedDict()   # key -> carrier; the last TAP_TABLE_CACHE keys: a request chooses its key
_carriers_on_device: collections.OrderedDict = collections.OrderedDict()   # (key, device) -> the carrier there
_tag_carriers_on_device: collections.OrderedDict = collections.OrderedDict()   # (key, device) -> its four rows there: its own, then its sub-keys'
_M64 = (1 << 64) - 1


def _check_key(key) -> int:
    if isinstance(key, (bool, np.bool_)) or not isinstance(key, (int, np.integer)) or not 1 <= int(key) <= WATERMARK_KEY_MAX:
        raise ValueError(f"watermark must be an integer key from 1 to 2^48 - 1 (got {key!r})")
    return int(key)


def check_watermark_id(value) -> int:
    """A trace id: an int in 0 .. 2^30 - 1; a bool, a float and a value out of range are a ValueError."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= WATERMARK_ID_MAX:
        raise ValueError(f"watermark id must be an integer from 0 to 2^30 - 1 (got {value!r})")
    return int(value)


def watermark_key(mark):
    """The key of a checked `watermark` value (an int or a `WatermarkTag`), None of None."""
    return mark.key if isinstance(mark, WatermarkTag) else mark


def check_watermark(key, default=None):
    """A request's `watermark` option: None (absent) stays None; an int in 1 .. 2^48 - 1 is the key; a bool, a float, a string and any
    other value are a ValueError.  `{"key": K, "id": I}` (or a `WatermarkTag`) is a key with a trace id, 0 .. 2^30 - 1, and gives
    `WatermarkTag(K, I)`; `{"id": I}` alone takes the key of `default` (a checked value: a service's own key) and is a ValueError without
    one; `{"key": K}` is the key K.  Any other entry of the dict is a ValueError that names it."""
    if key is None:
        return None
    if isinstance(key, WatermarkTag):
        key = {"key": key.key, "id": key.id}
    if isinstance(key, dict):
        unknown = [k for k in key if k not in ("key", "id")]
        if unknown:
            raise ValueError(f"watermark has an unknown entry {unknown[0]!r}: a key with a trace id is {{\"key\": K, \"id\": I}}")
        k, i = key.get("key"), key.get("id")
        if k is None:
            k = watermark_key(default)
            if k is None:
                raise ValueError(f"watermark names an id without a key, and the service has no key of its own (got {key!r})")
        k = _check_key(k)
        return k if i is None else WatermarkTag(k, check_watermark_id(i))
    return _check_key(key)


def check_watermark_keys(keys) -> list:
    """The keys a clip is scored against: 1 .. WATERMARK_KEYS_MAX of them, each an int by `check_watermark` (one key may stand for its
    list)."""
    if isinstance(keys, (int, np.integer)) and not isinstance(keys, (bool, np.bool_)):
        keys = [keys]
    if not isinstance(keys, (list, tuple)) or not 1 <= len(keys) <= WATERMARK_KEYS_MAX or any(k is None for k in keys):
        raise ValueError(f"watermark keys must be a list of 1 to {WATERMARK_KEYS_MAX} keys (got {keys!r})")
    return [_check_key(k) for k in keys]


def splitmix64(state: int):
    """(next state, output) of one SplitMix64 step."""
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def watermark_chips(key) -> np.ndarray:
    """The key's chips, int64 [WATERMARK_PERIOD] of +1 / -1."""
    state, words = check_watermark(key), []
    if state is None:
        raise ValueError("watermark_chips: a key is needed")
    for _ in range(WATERMARK_PERIOD // 64):
        state, z = splitmix64(state)
        words.append(z)
    bits = (np.asarray(words, dtype=np.uint64)[:, None] >> np.arange(64, dtype=np.uint64)[None]) & np.uint64(1)
    return bits.reshape(-1).astype(np.int64) * 2 - 1


def watermark_taps() -> np.ndarray:
    """The band taps g, int64 [WATERMARK_TAPS] (read-only)."""
    global _watermark_taps
    if _watermark_taps is None:
        k = np.arange(WATERMARK_TAPS, dtype=np.float64)
        half = WATERMARK_TAPS // 2
        hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * (k + 1.0) / (WATERMARK_TAPS + 1.0))
        hi, lo = 2.0 * 3200.0 / SAMPLE_RATE, 2.0 * 500.0 / SAMPLE_RATE
        g = np.rint(2.0 ** 14 * hann * (hi * np.sinc(hi * (k - half)) - lo * np.sinc(lo * (k - half)))).astype(np.int64)
        g.setflags(write=False)
        _watermark_taps = g
    return _watermark_taps


def watermark_carrier(key) -> np.ndarray:
    """The key's carrier c, int16 [WATERMARK_PERIOD] (read-only): its chips through the band taps, circularly.  The last
    TAP_TABLE_CACHE keys are kept."""
    key = check_watermark(key)
    hit = _lru_get(_watermark_carriers, key)
    if hit is None:
        chips, g, half = watermark_chips(key), watermark_taps(), WATERMARK_TAPS // 2
        ext = np.concatenate([chips[-half:], chips, chips[:half]])                   # ext[i] = chip[(i - 64) mod P]
        # c[m] = sum_k g[k] chip[m - k + 64] = sum_k g[k] ext[m + 128 - k]: a full convolution's samples 128 .. 128 + P - 1
        hit = (np.convolve(ext, g)[WATERMARK_TAPS - 1:WATERMARK_TAPS - 1 + WATERMARK_PERIOD] >> 3).astype(np.int16)
        hit.setflags(write=False)
        _lru_put(_watermark_carriers, key, hit)
    return hit


def _device_carrier(key, device):
    key = (check_watermark(key), str(device))
    hit = _lru_get(_carriers_on_device, key)
    return hit if hit is not None else _lru_put(_carriers_on_device, key, torch.from_numpy(watermark_carrier(key[0]).copy()).to(device))


def watermark_subkey(key, d) -> int:
    """Sub-key d (0 .. WATERMARK_ID_SYMBOLS - 1) of a key: an ordinary key, whose carrier holds symbol d of a trace id."""
    state = _check_key(key)
    if isinstance(d, (bool, np.bool_)) or not isinstance(d, (int, np.integer)) or not 0 <= d < WATERMARK_ID_SYMBOLS:
        raise ValueError(f"watermark_subkey: d is 0 .. {WATERMARK_ID_SYMBOLS - 1} (got {d!r})")
    for _ in range(WATERMARK_PERIOD // 64 + 1 + int(d)):                               # output number 257 + d
        state, z = splitmix64(state)
    return 1 + z % WATERMARK_KEY_MAX


def watermark_subkeys(key) -> list:
    return [watermark_subkey(key, d) for d in range(WATERMARK_ID_SYMBOLS)]


def watermark_id_symbols(value) -> list:
    """s_d of a trace id, d = 0 .. WATERMARK_ID_SYMBOLS - 1."""
    value = check_watermark_id(value)
    return [(value >> (_ID_SYMBOL_BITS * d)) & (_ID_SYMBOL_COUNT - 1) for d in range(WATERMARK_ID_SYMBOLS)]


def watermark_tag_carrier(mark) -> np.ndarray:
    """C of the definition above, int64 [WATERMARK_PERIOD]: 2 c_K, and with an id the three rotated sub-key carriers added."""
    mark = check_watermark(mark)
    C = 2 * watermark_carrier(watermark_key(mark)).astype(np.int64)
    if isinstance(mark, WatermarkTag):
        for sub, s in zip(watermark_subkeys(mark.key), watermark_id_symbols(mark.id)):
            C += np.roll(watermark_carrier(sub).astype(np.int64), WATERMARK_ID_STEP * s)   # roll(c, k)[m] = c[(m - k) mod P]
    return C


def _device_tag_carriers(key, device):
    """int16 [4, WATERMARK_PERIOD] on `device`: the key's carrier, then its sub-keys' 0 .. 2; the last TAP_TABLE_CACHE keys are kept, so a
    key seen before costs neither the sub-key arithmetic nor an upload."""
    key = (_check_key(key), str(device))
    hit = _lru_get(_tag_carriers_on_device, key)
    if hit is None:
        rows = np.stack([watermark_carrier(k) for k in [key[0]] + watermark_subkeys(key[0])])
        hit = _lru_put(_tag_carriers_on_device, key, torch.from_numpy(rows).to(device))
    return hit


def mark_pcm16(pcm, key) -> np.ndarray:
    """24 kHz int16 PCM [n] with the key's mark added, by the definitions above: integers only, the length kept, silence left silent.
    `key`: a key, or a `WatermarkTag` (or its dict) whose trace id the mark carries too; None returns the array itself.  What
    `ops.wave_mark` equals byte for byte."""
    pcm, key = _as_pcm16(pcm), check_watermark(key)
    if key is None or not len(pcm):
        return pcm
    n, B = len(pcm), WATERMARK_BLOCK
    x = pcm.astype(np.int64)
    A = np.add.reduceat(np.abs(x), np.arange(0, n, B))
    Ap = np.concatenate([[0], A, [0]])
    E = np.maximum(np.maximum(Ap[:-2], Ap[1:-1]), Ap[2:])
    j = np.arange(n)
    C = watermark_tag_carrier(key)              # a key alone: (E 2 c) >> 24 == (E c) >> 23
    return np.clip(x + ((E[j // B] * C[j % WATERMARK_PERIOD]) >> WATERMARK_ID_SHIFT), -32768, 32767).astype(np.int16)


def _watermark_samples(wave) -> np.ndarray:
    """A clip as the detector reads it: fp64 [n], int16 scaled by 1 / 32768, only the first WATERMARK_MAX_SAMPLES samples."""
    if torch.is_tensor(wave):
        wave = wave.detach().cpu().numpy()
    wave = np.asarray(wave)
    if wave.dtype == np.int16:
        x = wave.reshape(-1)[:WATERMARK_MAX_SAMPLES].astype(np.float64) / 32768.0
    elif np.issubdtype(wave.dtype, np.floating):
        x = wave.reshape(-1)[:WATERMARK_MAX_SAMPLES].astype(np.float64)
    else:
        raise ValueError(f"detect_watermark: the clip is int16 PCM or floating-point samples (got {wave.dtype})")
    if not np.isfinite(x).all():
        raise ValueError("detect_watermark: the clip has a sample that is not finite")
    return x


def watermark_fold(wave) -> np.ndarray:
    """Z of the definition above, fp64 [WATERMARK_PERIOD]: the clip's whitened band, folded by the period."""
    x = _watermark_samples(wave)
    n, N, H, pad = len(x), 1024, 256, 768
    F = -(-(n + pad) // H)
    w = np.sin(np.pi * np.arange(N) / N)
    xp = np.zeros(H * (F - 1) + N)
    xp[pad:pad + n] = x
    X = np.fft.rfft(np.lib.stride_tricks.sliding_window_view(xp, N)[::H] * w, axis=1)
    U = np.zeros_like(X)
    lo, hi = WATERMARK_BAND
    band = X[:, lo:hi + 1]
    U[:, lo:hi + 1] = band / np.sqrt(band.real ** 2 + band.imag ** 2 + 1e-10)
    y = np.fft.irfft(U, n=N, axis=1) * w
    u = np.zeros_like(xp)
    for m in range(F):
        u[H * m:H * m + N] += y[m]
    u = u[pad:pad + n]
    Z = np.zeros(-(-n // WATERMARK_PERIOD) * WATERMARK_PERIOD)
    Z[:n] = u
    return Z.reshape(-1, WATERMARK_PERIOD).sum(axis=0)


def watermark_score(r, key) -> WatermarkScore:
    """The score of a key from its correlation r [WATERMARK_PERIOD] over the offsets."""
    o = int(np.argmax(r))                       # the smallest argmax
    sigma = float(np.std(r))
    z = (float(r[o]) - float(np.mean(r))) / sigma if sigma > 0 else 0.0
    return WatermarkScore(key, z, o, bool(z >= WATERMARK_THRESHOLD))


def detect_watermark(wave, keys) -> list:
    """One `WatermarkScore(key, z, offset, detected)` per key for a mono 24 kHz clip, int16 PCM or float samples (scored in fp64), by the
    definition above; a clip below WATERMARK_MIN_SAMPLES scores z = 0 and is not detected.  The correlation over all offsets is formed
    with fp64 FFTs."""
    keys = check_watermark_keys(keys)
    x = _watermark_samples(wave)
    if len(x) < WATERMARK_MIN_SAMPLES:
        return [WatermarkScore(k, 0.0, 0, False) for k in keys]
    FZ = np.conj(np.fft.rfft(watermark_fold(x)))
    return [watermark_score(np.fft.irfft(FZ * np.fft.rfft(watermark_carrier(k).astype(np.float64)), n=WATERMARK_PERIOD), k) for k in keys]


def watermark_symbol(r, offset):
    """(s_d, z_d) of a sub-key from its correlation r [WATERMARK_PERIOD] and the key's offset o*."""
    grid = (offset - WATERMARK_ID_STEP * np.arange(_ID_SYMBOL_COUNT)) % WATERMARK_PERIOD
    s = int(np.argmax(r[grid]))                 # the smallest argmax
    sigma = float(np.std(r))
    return s, (float(r[grid[s]]) - float(np.mean(r))) / sigma if sigma > 0 else 0.0


def watermark_read(score, symbols) -> WatermarkRead:
    """The `WatermarkRead` of a key from its `WatermarkScore` and its three (s_d, z_d): the id only when the key is detected and every
    z_d >= WATERMARK_ID_THRESHOLD."""
    id_z = min(z for _, z in symbols)
    found = score.detected and all(z >= WATERMARK_ID_THRESHOLD for _, z in symbols)
    value = sum(int(s) << (_ID_SYMBOL_BITS * d) for d, (s, _) in enumerate(symbols)) if found else None
    return WatermarkRead(score.key, score.z, score.offset, score.detected, value, float(id_z))


def read_watermark(wave, keys) -> list:
    """One `WatermarkRead(key, z, offset, detected, id, id_z)` per key for a mono 24 kHz clip: `detect_watermark`'s score of the key, and
    the trace id its mark carries (None when the key is not detected or a symbol stays below WATERMARK_ID_THRESHOLD) with the smallest
    symbol score, by the definition above.  A clip below WATERMARK_MIN_SAMPLES reads z = 0, id None, id_z = 0."""
    keys = check_watermark_keys(keys)
    x = _watermark_samples(wave)
    if len(x) < WATERMARK_MIN_SAMPLES:
        return [WatermarkRead(k, 0.0, 0, False, None, 0.0) for k in keys]
    FZ = np.conj(np.fft.rfft(watermark_fold(x)))
    corr = lambda k: np.fft.irfft(FZ * np.fft.rfft(watermark_carrier(k).astype(np.float64)), n=WATERMARK_PERIOD)
    out = []
    for k in keys:
        score = watermark_score(corr(k), k)
        out.append(watermark_read(score, [watermark_symbol(corr(sub), score.offset) for sub in watermark_subkeys(k)]))
    return out


# Scan: where in a long or spliced recording the marked stretches lie, and which trace id each carries (`scan_watermark`).  `detect_watermark`
# folds one whole clip of at most 60 s at one phase; stretches cut together have different phases and cancel, and anything past 60 s is not
# read.  The mark, the chips, the carriers and the id arithmetic above stay; the scan folds WINDOWS of the recording.
#   constants  WATERMARK_SCAN_WINDOW W = 2 periods per window, WATERMARK_SCAN_SLACK = 2 samples, WATERMARK_SCAN_MAX_SAMPLES = 14 400 000
#              (600 s: the cap FLAC_MAX_SECONDS puts on an upload); P = WATERMARK_PERIOD
#   whitening  u = the whitened band of the WHOLE recording by `watermark_fold`'s framing -- 768 zeros in front, frames of 1024 at hop 256,
#              the sine window, the unit-modulus band, overlap-add in ascending frame order --, cropped to the n samples
#              (`watermark_whitened`: frames are independent, so it works in slabs of 2048 frames, 16 MB of fp64 each)
#   segments   S = ceil(n / P); segment s is u[s P .. (s + 1) P), the last one zero-filled
#   windows    max(1, S - W + 1) of them (`watermark_windows`); window w covers segments w .. min(w + W, S) - 1; its row is
#              Z_w[m] = sum over its segments, ascending, of u[s P + m].  A segment starts at a multiple of P, so this is the fold of those
#              samples by their ABSOLUTE index: a reported offset refers to sample 0 of the recording, as `detect_watermark`'s does
#   score      per key, `watermark_score` of r[o] = sum_m Z_w[m] c[(m + o) mod P]: the same formula, the smallest argmax, detected at
#              z >= 7.0
#   spans      `watermark_spans`, per key: a span is a maximal run of consecutive detected windows a .. b in which each window's offset lies
#              within WATERMARK_SCAN_SLACK of the previous window's, circularly mod P.  It covers segments a .. min(b + W, S) - 1:
#              start = a P, end = min(n, (b + W) P), in samples
#   read       Z_span = the sum of the span's segment rows, ascending; `watermark_score` of the key's correlation on it gives the span's z
#              and offset, `watermark_symbol` of the three sub-keys at that offset the symbols, and `watermark_read` decides the id
#              (z >= 7.0 and every z_d >= 6.0), exactly as `read_watermark` does.  A span whose own fold scores z < 7.0 is DROPPED: its
#              windows agreed one by one, but their sum does not carry the key
#   result     `WatermarkSpan(key, start, end, z, offset, id, id_z)`, sorted by (start, the key's position in `keys`)
#   input      dtypes and the finite check are `detect_watermark`'s; n < WATERMARK_MIN_SAMPLES gives []; n > WATERMARK_SCAN_MAX_SAMPLES
#              is a ValueError that names both numbers: this function never truncates
# Properties: a span's edges are whole segments, so it exceeds the marked stretch by less than two periods (1.37 s) at either end; a
# marked stretch shorter than about one period may be missed (no window holds enough of it); false alarms are about 5e-9 per (window, key),
# 878 windows in 600 s.  Every figure comes from synthetic speech-like hosts; nobody has measured real speech.
WATERMARK_SCAN_WINDOW = 2
WATERMARK_SCAN_SLACK = 2
WATERMARK_SCAN_MAX_SAMPLES = 14_400_000
WatermarkSpan = collections.namedtuple("WatermarkSpan", "key start end z offset id id_z")
WatermarkRange = collections.namedtuple("WatermarkRange", "key first count start end")   # a span before it is read: segments first .. first + count - 1
_SCAN_FRAME_SLAB = 2048


def _scan_samples(wave) -> np.ndarray:
    """A recording as the scan reads it: `detect_watermark`'s dtypes and finite check, but every sample; past the cap a ValueError."""
    if torch.is_tensor(wave):
        wave = wave.detach().cpu().numpy()
    wave = np.asarray(wave)
    n = wave.size
    if n > WATERMARK_SCAN_MAX_SAMPLES:
        raise ValueError(f"scan_watermark: the recording has {n} samples; at most {WATERMARK_SCAN_MAX_SAMPLES} (600 s at 24 kHz) are scanned")
    if wave.dtype == np.int16:
        x = wave.reshape(-1).astype(np.float64) / 32768.0
    elif np.issubdtype(wave.dtype, np.floating):
        x = wave.reshape(-1).astype(np.float64)
    else:
        raise ValueError(f"detect_watermark: the clip is int16 PCM or floating-point samples (got {wave.dtype})")
    if not np.isfinite(x).all():
        raise ValueError("detect_watermark: the clip has a sample that is not finite")
    return x


def watermark_whitened(x) -> np.ndarray:
    """u of the scan's definition, fp64 [n]: the whitened band of fp64 samples x [n] by `watermark_fold`'s framing, frame slab by frame
    slab (the host never holds more than _SCAN_FRAME_SLAB frames beside x and u)."""
    x = np.asarray(x, dtype=np.float64)
    n, N, H, pad = len(x), 1024, 256, 768
    F = -(-(n + pad) // H)
    w = np.sin(np.pi * np.arange(N) / N)
    xp = np.zeros(H * (F - 1) + N)
    xp[pad:pad + n] = x
    frames = np.lib.stride_tricks.sliding_window_view(xp, N)[::H]
    u = np.zeros(H * (F + N // H - 1)).reshape(-1, H)                                  # hop blocks: frame m adds to blocks m .. m + 3
    lo, hi = WATERMARK_BAND
    for m0 in range(0, F, _SCAN_FRAME_SLAB):
        m1 = min(F, m0 + _SCAN_FRAME_SLAB)
        X = np.fft.rfft(frames[m0:m1] * w, axis=1)
        U = np.zeros_like(X)
        band = X[:, lo:hi + 1]
        U[:, lo:hi + 1] = band / np.sqrt(band.real ** 2 + band.imag ** 2 + 1e-10)
        y = (np.fft.irfft(U, n=N, axis=1) * w).reshape(m1 - m0, N // H, H)
        for d in range(N // H - 1, -1, -1):                                           # block b takes frames b - 3 .. b: ascending frame order
            u[m0 + d:m1 + d] += y[:, d]
    return u.reshape(-1)[pad:pad + n]


def watermark_windows(n) -> int:
    """Windows of a recording of n samples: max(1, S - W + 1), S = ceil(n / P)."""
    return max(1, -(-int(n) // WATERMARK_PERIOD) - WATERMARK_SCAN_WINDOW + 1)


def watermark_spans(scores, n) -> list:
    """The spans of the scan's definition from the window scores alone: `scores[w]` holds window w's `WatermarkScore`s, one per key in the
    keys' order, for all `watermark_windows(n)` windows of a recording of n samples.  Returns `WatermarkRange(key, first, count, start,
    end)`s -- segments first .. first + count - 1, samples [start, end) -- sorted by (start, the key's position).  Pure: no audio is read."""
    P, W = WATERMARK_PERIOD, WATERMARK_SCAN_WINDOW
    S = -(-int(n) // P)
    if len(scores) != watermark_windows(n):
        raise ValueError(f"watermark_spans: a recording of {n} samples has {watermark_windows(n)} windows (got {len(scores)} score rows)")
    out = []
    for k in range(len(scores[0]) if len(scores) else 0):
        a = prev = None                                             # the open run's first window and its last window's offset
        for w in range(len(scores) + 1):
            s = scores[w][k] if w < len(scores) else None
            d = None if s is None or prev is None else (s.offset - prev) % P
            if a is not None and (s is None or not s.detected or min(d, P - d) > WATERMARK_SCAN_SLACK):
                last = min(w - 1 + W, S)                            # the run a .. w - 1 ends: one segment past its last one
                out.append((a * P, k, WatermarkRange(scores[a][k].key, a, last - a, a * P, min(int(n), last * P))))
                a = None
            if s is not None and s.detected:
                if a is None:
                    a = w
                prev = s.offset
            else:
                prev = None
    return [r for _, _, r in sorted(out, key=lambda t: t[:2])]


def _scan_correlations(Z, carriers) -> np.ndarray:
    """r [len(carriers), rows, P] of fold rows Z [rows, P] against int16 carriers, with fp64 FFTs as `detect_watermark` forms it."""
    FZ = np.conj(np.fft.rfft(Z, axis=1))
    return np.stack([np.fft.irfft(FZ * np.fft.rfft(c.astype(np.float64)), n=WATERMARK_PERIOD, axis=1) for c in carriers])


def scan_segment_rows(x) -> np.ndarray:
    """The segment rows [S, P] of fp64 samples x: u, zero-filled to whole periods."""
    P = WATERMARK_PERIOD
    n = len(x)
    S = -(-n // P)
    seg = np.zeros(S * P)
    seg[:n] = watermark_whitened(x)
    return seg.reshape(S, P)


def _window_rows(seg, w0, w1) -> np.ndarray:
    """Z_w [w1 - w0, P] of windows w0 .. w1 - 1 from the segment rows: each the sum of its segments in ascending order."""
    S, rows = len(seg), []
    for w in range(w0, w1):
        acc = seg[w].copy()
        for s in range(w + 1, min(w + WATERMARK_SCAN_WINDOW, S)):
            acc += seg[s]
        rows.append(acc)
    return np.stack(rows)


def scan_window_rows(x) -> tuple:
    """(segment rows [S, P], window rows Z_w [windows, P]) of fp64 samples x, by the scan's definition."""
    seg = scan_segment_rows(x)
    return seg, _window_rows(seg, 0, watermark_windows(len(x)))


def scan_watermark(wave, keys) -> list:
    """Where a mono 24 kHz recording (int16 PCM or float samples, up to 600 s) carries the marks of `keys`, by the definition above: one
    `WatermarkSpan(key, start, end, z, offset, id, id_z)` per marked stretch and key -- start and end in samples, whole periods outwards of
    the stretch by less than two; z and offset of the span's own fold, the offset relative to sample 0 of the recording; id the trace id the
    stretch carries or None, id_z its smallest symbol score -- sorted by (start, the key's position in `keys`).  [] below
    WATERMARK_MIN_SAMPLES; ValueError above WATERMARK_SCAN_MAX_SAMPLES (never truncated).  fp64, frame slab by frame slab."""
    keys = check_watermark_keys(keys)
    x = _scan_samples(wave)
    n = len(x)
    if n < WATERMARK_MIN_SAMPLES:
        return []
    seg = scan_segment_rows(x)
    scores, out, windows = [], [], watermark_windows(n)
    for w0 in range(0, windows, 64):                                # (64 windows at a time: 8 MB of correlations per key)
        r = _scan_correlations(_window_rows(seg, w0, min(w0 + 64, windows)), [watermark_carrier(k) for k in keys])
        scores += [[watermark_score(r[i, w], k) for i, k in enumerate(keys)] for w in range(r.shape[1])]
    for g in watermark_spans(scores, n):
        Z = seg[g.first].copy()
        for s in range(g.first + 1, g.first + g.count):
            Z += seg[s]
        rk = _scan_correlations(Z[None], [watermark_carrier(k) for k in [g.key] + watermark_subkeys(g.key)])[:, 0]
        score = watermark_score(rk[0], g.key)
        if not score.detected:
            continue                                                # the span's own fold does not carry the key: dropped
        read = watermark_read(score, [watermark_symbol(rk[1 + d], score.offset) for d in range(WATERMARK_ID_SYMBOLS)])
        out.append(WatermarkSpan(g.key, g.start, g.end, read.z, read.offset, read.id, read.id_z))
    return out


_G711_TAGS = {"mulaw": 7, "alaw": 6}   # WAVE_FORMAT_MULAW, WAVE_FORMAT_ALAW


def _g711_header(encoding, sample_rate, n, riff_size, data_size):
    """RIFF header of a mono G.711 WAV: an 18-byte `fmt ` chunk (format tag 7 / 6, 8 bits per sample, block align 1, byte rate = sample rate,
    cbSize 0), a `fact` chunk with the sample count, and the `data` chunk's header."""
    return (b"RIFF" + struct.pack("<I", riff_size) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHHH", 18, _G711_TAGS[encoding], 1, sample_rate, sample_rate, 1, 8, 0)
            + b"fact" + struct.pack("<II", 4, n) + b"data" + struct.pack("<I", data_size))


def delivery_bytes(audio, encoding: str = "pcm16") -> bytes:
    """The body bytes of samples in any of the forms a request's result takes: uint8 G.711 codes or FLAC stream bytes as they are, int16
    PCM little-endian, float samples by `pcm16`'s rule -- and, for a G.711 `encoding`, PCM that is not encoded yet through `encode_g711`
    ("flac" needs the rate as well: `encode_flac`)."""
    a = np.asarray(audio)
    if a.dtype == np.uint8:
        return a.tobytes()
    if encoding in FLAC_ENCODINGS:
        raise ValueError("delivery_bytes: a FLAC body is the stream `encode_flac` / `deliver_pcm16` made (uint8), not samples")
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


# ----------------------------------------- FLAC (RFC 9639), the fixed-predictor subset: the one compressed delivery format, lossless, integer
# arithmetic with no freedom left once the choice rule is written down -- so the device encoder (csrc/wave_out.h wave_flac_*) is held to
# `encode_flac` byte for byte like every other back-end kernel.
#   stream    "fLaC", one STREAMINFO block (last-block flag, length 34): min = max block size 4096, the true min / max frame size and total
#             sample count, MD5 all zero ("not computed": a device-side result must not need the PCM on the host); 42 bytes; then the frames
#   frame     sync 0xFFF8 (fixed block size: the FRAME number is coded), block-size code 1100 (4096) or, for the short last frame, 0111 with a
#             16-bit b - 1; the rate's code; channel code 0000; sample-size code 100; the frame number UTF-8-like; CRC-8; ONE subframe without
#             wasted bits; zero padding to a byte; CRC-16
#   subframe  CONSTANT when all samples of the block are equal; else the fixed order o in 0..4, o < b, with the fewest bits (ties: the lower
#             order); VERBATIM only when strictly smaller than that.  Bits: CONSTANT 8 + 16, VERBATIM 8 + 16 b, FIXED 8 + 16 o + 2 + 4 +
#             sum over partitions (4 + S_k)
#   residual  coding method 00 (4-bit Rice parameters), never the escape code; a full block has partition order 4 (16 partitions of 256, the
#             first with 256 - o residuals), the short last block partition order 0; per partition k in 0..14 minimises S_k = sum(u >> k) +
#             n (1 + k) (ties: the smaller k), u = 2 r for r >= 0 and -2 r - 1 otherwise; a code is u >> k zero bits, a one, the low k bits
#
# Level 1 (`encode_flac(pcm, rate, level=1)`, a request's `flac_level`) adds LPC subframes to the candidates of every FULL block that is not
# constant; everything else above -- stream and frame headers, the CONSTANT test, the short last block (level-0 rule only), coding method 00,
# partition order 4, the Rice parameter rule -- stays.  The candidates in order: FIXED 0, 1, 2, 3, 4, then LPC order 6, 8, 10, 12, made so
# (csrc/flac_lpc_core.h is the same text for the kernel and for tools/flac_lpc_check.cpp):
#   window    w[i] = (32768 (4095^2 - (2 i - 4095)^2)) // 4095^2, a Welch window in integers; xw[i] = (x[i] w[i]) >> 15 (arithmetic)
#   autocorr  R[j] = sum_{i >= j} xw[i] xw[i - j], j in 0..12, exact integers (below 2^43); R[0] == 0: no LPC candidates
#   Levinson  in fp64, every step ONE correctly rounded operation in this order, no fused multiply-add, no reassociation:
#             err = double(R[0]); for m = 1..12: acc = double(R[m]); for j = 0..m-2: acc = acc - a[j] * double(R[m-1-j]); k = acc / err;
#             a'[j] = a[j] - k * a[m-2-j] for j < m-1, a'[m-1] = k; err = err * (1.0 - k * k); if not err > 0.0, order m and every higher
#             order are no candidates.  Order m's coefficients are a[0..m-1] after step m; a[0] multiplies the most recent sample
#   quantise  12 bits: cmax = max |a[j]|, e = frexp(cmax)'s exponent (0 for cmax = 0), shift = min(11 - e, 15), shift < 0: no candidate;
#             q[j] = clip(rint(a[j] 2^shift), -2048, 2047), rint to even, the scaling exact.  (An order with a coefficient that is not finite is no
#             candidate.  It cannot be reached -- err > 0 keeps |k| < 1 -- and is decided here so that both sides agree.)
#   residual  r[i] = x[i] - ((sum_j q[j] x[i-1-j]) >> shift), i >= o, arithmetic shift; the sum stays below 12 2048 32768 < 2^31.  GUARD: an
#             order with any zigzag u >= 2^21 is no candidate, which keeps every partition sum sum(u >> k) below 2^29 (exact in 32 bits)
#   bits      8 + 16 o + 4 + 5 + 12 o + 2 + 4 + sum over partitions (4 + S_k), the first partition with 256 - o residuals
#   choice    the fewest bits, ties to the earlier candidate of the list; VERBATIM only when strictly smaller, CONSTANT as before -- so a
#             level-1 frame is never larger than the level-0 frame of the same block
#   on wire   subframe header byte (0x20 | (o - 1)) << 1, o warm-up samples of 16 bits, 0b1011 (precision - 1), the shift in 5 signed bits,
#             o coefficients of 12 signed bits (q[0] first), then the residual section exactly as in a FIXED subframe
FLAC_BLOCK = 4096
FLAC_HEADER_BYTES = 42
FLAC_RATE_CODES = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}
FLAC_LEVELS = (0, 1)
FLAC_LPC_ORDERS = (6, 8, 10, 12)
FLAC_LPC_PRECISION = 12
FLAC_LPC_GUARD = 1 << 21
_FLAC_MAX_K = 14
_FLAC_PARTITION_ORDER = 4
_FLAC_VERBATIM = 5                                # `_flac_plan`'s kinds: -1 CONSTANT, 0..4 FIXED, 5 VERBATIM, 6 + i LPC of FLAC_LPC_ORDERS[i]


def check_flac_level(level) -> int:
    """A FLAC level as an int: 0 or 1, not a bool; None is 0."""
    if level is None:
        return 0
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or int(level) not in FLAC_LEVELS:
        raise ValueError(f"flac_level must be one of {list(FLAC_LEVELS)} (got {level!r})")
    return int(level)


def request_flac_level(flac_level, encoding) -> int:
    """`check_flac_level` for a request: a level beside an encoding that is not FLAC is refused, never ignored."""
    level = check_flac_level(flac_level)
    if flac_level is not None and (encoding if encoding is not None else "pcm16") not in FLAC_ENCODINGS:
        raise ValueError(f"flac_level needs encoding 'flac' (got flac_level {flac_level!r} with encoding {encoding!r})")
    return level


def _crc_table(poly, bits):
    top, mask, table = 1 << (bits - 1), (1 << bits) - 1, []
    for b in range(256):
        c = b << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        table.append(c)
    return table


_CRC8_TABLE, _CRC16_TABLE = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def flac_crc8(data) -> int:
    """CRC-8 of a frame header: polynomial 0x07, initial value 0 (of b"123456789": 0xF4)."""
    c = 0
    for b in bytes(data):
        c = _CRC8_TABLE[c ^ b]
    return c


def flac_crc16(data) -> int:
    """CRC-16 of a frame: polynomial 0x8005, initial value 0, not reflected (of b"123456789": 0xFEE8)."""
    c, t = 0, _CRC16_TABLE
    for b in bytes(data):
        c = ((c << 8) & 0xFFFF) ^ t[(c >> 8) ^ b]
    return c


def _flac_number(v):
    """A frame number in the format's UTF-8-like coding: 7 bits in one byte, else 11, 16, 21, 26, 31 or 36 bits in 2 .. 7."""
    if v < 0x80:
        return bytes([v])
    n = 2
    while n < 7 and v >= 1 << (5 * n + 1):
        n += 1
    lead = (0xFF << (8 - n)) & 0xFF
    return bytes([lead | (v >> (6 * (n - 1)))] + [0x80 | ((v >> (6 * k)) & 0x3F) for k in range(n - 2, -1, -1)])


def _flac_rate(sample_rate):
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or int(sample_rate) not in FLAC_RATE_CODES:
        raise ValueError(f"sample_rate must be one of {list(OUTPUT_SAMPLE_RATES)} (got {sample_rate!r})")
    return int(sample_rate)


def flac_stream_header(sample_rate, total=0, min_frame=0, max_frame=0) -> bytes:
    """The 42 bytes in front of the frames: "fLaC" and STREAMINFO (mono, 16 bits, block size 4096, MD5 zero); zeros mean "unknown"."""
    rate = _flac_rate(sample_rate)
    info = (struct.pack(">HH", FLAC_BLOCK, FLAC_BLOCK) + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big")
            + ((rate << 44) | (0 << 41) | (15 << 36) | total).to_bytes(8, "big") + bytes(16))
    return b"fLaC" + bytes([0x80]) + len(info).to_bytes(3, "big") + info


def _flac_rice(u, o, parts, plen):
    """(ks [F, parts], S [F, parts]) of zigzag residuals u [F, b - o]: per partition the parameter that minimises S_k, and that minimum."""
    F = u.shape[0]
    padded = np.concatenate([np.zeros((F, o), dtype=np.int64), u], axis=1).reshape(F, parts, plen)       # (a zero adds nothing to sum(u >> k))
    n = np.full(parts, plen, dtype=np.int64)
    n[0] -= o
    s = np.stack([(padded >> k).sum(axis=2) + n * (1 + k) for k in range(_FLAC_MAX_K + 1)])            # [15, F, parts]
    return s.argmin(axis=0), s.min(axis=0)                                                              # (the first minimum: the smaller k)


def flac_lpc_window() -> np.ndarray:
    """The level-1 window, int64 [4096]: a Welch window at 2^15 in integers."""
    i = np.arange(FLAC_BLOCK, dtype=np.int64)
    m = FLAC_BLOCK - 1
    return (32768 * (m * m - (2 * i - m) ** 2)) // (m * m)


def flac_lpc_autocorrelation(x) -> np.ndarray:
    """R int64 [F, 13] of full blocks x int64 [F, 4096]: the windowed autocorrelation, exact."""
    xw = (x * flac_lpc_window()) >> 15
    return np.stack([(xw[:, j:] * xw[:, :FLAC_BLOCK - j]).sum(axis=1) for j in range(FLAC_LPC_ORDERS[-1] + 1)], axis=1)


def flac_lpc_coefficients(R):
    """{order: (q, shift)} of one block's autocorrelation R (13 ints): Levinson-Durbin and the quantisation of the level-1 rule, for the
    orders that are candidates so far.  Scalar float64 arithmetic in a plain loop: one rounding per operation, in the written order."""
    out = {}
    R = [int(v) for v in R]
    if R[0] == 0:
        return out
    Rf = [float(v) for v in R]
    err, a = Rf[0], []
    for m in range(1, FLAC_LPC_ORDERS[-1] + 1):
        acc = Rf[m]
        for j in range(m - 1):
            acc = acc - a[j] * Rf[m - 1 - j]
        k = acc / err
        a = [a[j] - k * a[m - 2 - j] for j in range(m - 1)] + [k]
        err = err * (1.0 - k * k)
        if not err > 0.0:
            break
        if m in FLAC_LPC_ORDERS:
            if not all(math.isfinite(v) for v in a):
                continue
            cmax = max(abs(v) for v in a)
            shift = min(FLAC_LPC_PRECISION - 1 - math.frexp(cmax)[1], 15)
            if shift < 0:
                continue
            lim = 1 << (FLAC_LPC_PRECISION - 1)
            out[m] = ([min(max(int(round(math.ldexp(v, shift))), -lim), lim - 1) for v in a], shift)      # (round: half to even)
    return out


def flac_lpc_residual(x, q, shift):
    """The zigzag residuals u int64 [F, 4096 - o] of blocks x int64 [F, 4096] under per-block coefficients q int64 [F, o] and shifts [F], and
    the guard per block: False where some u reaches FLAC_LPC_GUARD (that order is no candidate for that block)."""
    F, b = x.shape
    o = q.shape[1]
    pred = np.zeros((F, b - o), dtype=np.int64)
    for j in range(o):
        pred += q[:, j:j + 1] * x[:, o - 1 - j:b - 1 - j]
    r = x[:, o:] - (pred >> np.asarray(shift, dtype=np.int64).reshape(F, 1))
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    return u, u.max(axis=1) < FLAC_LPC_GUARD


def _flac_plan(x, level=0):
    """The choice rule on blocks x int64 [F, b] of one size: (kind [F]: -1 CONSTANT, 0..4 the fixed order, 5 VERBATIM, 6 + i LPC of order
    FLAC_LPC_ORDERS[i]; ks [F, P]: the chosen candidate's Rice parameters; us: per candidate the zigzag residuals [F, b - o]; lpc: per LPC
    order (q [F, o], shift [F]), empty at level 0 and for a short block).  About 75 passes over the blocks: 5 orders x 15 parameters, and
    60 more at level 1."""
    F, b = x.shape
    parts = 1 << _FLAC_PARTITION_ORDER if b == FLAC_BLOCK else 1
    plen = b // parts
    orders = min(5, b)
    bits, ks, us, lpc, r = [], [], [], [], x
    for o in range(orders):
        if o:
            r = np.diff(r, axis=1)
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        us.append(u)
        k, s = _flac_rice(u, o, parts, plen)
        ks.append(k)
        bits.append(8 + 16 * o + 2 + 4 + (4 + s).sum(axis=1))
    if level and b == FLAC_BLOCK and F:
        coefs = [flac_lpc_coefficients(R) for R in flac_lpc_autocorrelation(x)]
        for o in FLAC_LPC_ORDERS:
            q, shift = np.zeros((F, o), dtype=np.int64), np.zeros(F, dtype=np.int64)
            valid = np.zeros(F, dtype=bool)
            for f, c in enumerate(coefs):
                if o in c:
                    q[f], shift[f], valid[f] = c[o][0], c[o][1], True
            u, inside = flac_lpc_residual(x, q, shift)
            valid &= inside
            u = np.where(valid[:, None], u, 0)
            k, s = _flac_rice(u, o, parts, plen)
            us.append(u)
            ks.append(k)
            lpc.append((q, shift))
            bits.append(np.where(valid, 8 + 16 * o + 4 + 5 + FLAC_LPC_PRECISION * o + 2 + 4 + (4 + s).sum(axis=1), np.iinfo(np.int64).max))
    bits, ks = np.stack(bits), np.stack(ks)
    cand = bits.argmin(axis=0)                                                                          # (the first minimum: the earlier candidate)
    best = bits[cand, np.arange(F)]
    kind = np.where(cand >= 5, cand + 1, cand)
    kind = np.where(8 + 16 * b < best, _FLAC_VERBATIM, kind)
    kind = np.where((x == x[:, :1]).all(axis=1), -1, kind)
    return kind, ks[cand, np.arange(F)], us, lpc


def _be16_bits(v):
    return np.unpackbits(np.asarray(v).astype(">i2").view(np.uint8))


def _signed_bits(v, width):
    """The `width`-bit two's complement of ints v, most significant bit first, as a flat uint8 array of bits."""
    v = np.asarray(v, dtype=np.int64).reshape(-1, 1) & ((1 << width) - 1)
    return ((v >> np.arange(width - 1, -1, -1)) & 1).astype(np.uint8).reshape(-1)


def _flac_frame(x, number, rate_code, kind, ks, u, lpc=None):
    """One frame's bytes: block x (int64 [b]) as frame `number`, with `_flac_plan`'s choice for it (u: the chosen candidate's residuals;
    lpc: (q, shift) of an LPC choice)."""
    b = len(x)
    head = bytes([0xFF, 0xF8, ((0x0C if b == FLAC_BLOCK else 0x07) << 4) | rate_code, 0x08]) + _flac_number(number)
    if b != FLAC_BLOCK:
        head += (b - 1).to_bytes(2, "big")
    head += bytes([flac_crc8(head)])
    if kind == -1:
        body = bytes([0x00]) + int(x[0]).to_bytes(2, "big", signed=True)
    elif kind == _FLAC_VERBATIM:
        body = bytes([0x02]) + x.astype(">i2").tobytes()
    else:
        o = int(kind) if lpc is None else len(lpc[0])
        parts = len(ks)
        plen = b // parts
        k = np.repeat(ks, plen)[o:]
        q = u >> k
        length = q + 1 + k
        extra = 0 if lpc is None else 4 + 5 + FLAC_LPC_PRECISION * o     # precision, shift and coefficients of an LPC subframe
        lead = 8 + 16 * o + extra + 6                             # subframe header, warm-up, coding method and partition order
        bounds = np.concatenate([[0], np.cumsum(length)])        # code i starts at bounds[i] + lead + 4 * (partitions opened up to it)
        opened = np.repeat(np.arange(1, parts + 1), plen)[o:]
        start = lead + 4 * opened + bounds[:-1]
        nbits = lead + 4 * parts + int(bounds[-1])
        bit = np.zeros((nbits + 7) // 8 * 8, dtype=np.uint8)
        bit[:8] = np.unpackbits(np.array([((8 | o) if lpc is None else (0x20 | (o - 1))) << 1], dtype=np.uint8))
        bit[8:8 + 16 * o] = _be16_bits(x[:o])
        if lpc is not None:
            at = 8 + 16 * o
            bit[at:at + 4] = _signed_bits(FLAC_LPC_PRECISION - 1, 4)
            bit[at + 4:at + 9] = _signed_bits(lpc[1], 5)
            bit[at + 9:at + 9 + FLAC_LPC_PRECISION * o] = _signed_bits(lpc[0], FLAC_LPC_PRECISION)
        bit[lead - 4:lead] = np.unpackbits(np.array([_FLAC_PARTITION_ORDER if parts > 1 else 0], dtype=np.uint8))[4:]
        first = np.concatenate([[0], np.arange(1, parts) * plen - o])          # the first residual of each partition
        pstart = start[first] - 4
        for j in range(4):
            bit[pstart + j] = (ks >> (3 - j)) & 1
        bit[start + q] = 1
        for j in range(_FLAC_MAX_K):                              # low bit j of the codes whose parameter reaches it, most significant first
            m = k > j
            bit[(start + q + 1 + j)[m]] = ((u[m] >> (k[m] - 1 - j)) & 1).astype(np.uint8)
        body = np.packbits(bit).tobytes()
    frame = head + body
    return frame + flac_crc16(frame).to_bytes(2, "big")


def _flac_frames(pcm, first_number, rate_code, level=0):
    """The frames of int16 PCM whose first block is frame `first_number`: whole blocks of 4096 and, if samples remain, one short block."""
    n = len(pcm)
    full, out = n // FLAC_BLOCK, []
    groups = [pcm[:full * FLAC_BLOCK].astype(np.int64).reshape(full, FLAC_BLOCK)] if full else []
    if n % FLAC_BLOCK:
        groups.append(pcm[full * FLAC_BLOCK:].astype(np.int64)[None])
    for x in groups:
        const = (x == x[:, :1]).all(axis=1)                       # (not planned: a long silence costs one comparison per sample)
        busy = np.flatnonzero(~const)
        kind, ks, us, lpc = _flac_plan(x[busy], level) if len(busy) else (None, None, None, None)
        where = {int(f): i for i, f in enumerate(busy)}
        for f in range(len(x)):
            number = first_number + len(out)
            if const[f]:
                out.append(_flac_frame(x[f], number, rate_code, -1, None, None))
                continue
            i, kd = where[f], int(kind[where[f]])
            if kd > _FLAC_VERBATIM:
                c = kd - 1
                out.append(_flac_frame(x[f], number, rate_code, kd, ks[i], us[c][i], (lpc[c - 5][0][i], int(lpc[c - 5][1][i]))))
            else:
                out.append(_flac_frame(x[f], number, rate_code, kd, ks[i], us[kd][i] if 0 <= kd < 5 else None))
    return out


def encode_flac(pcm, sample_rate, level=0) -> np.ndarray:
    """The native FLAC stream (uint8) of mono int16 PCM at `sample_rate` (one of OUTPUT_SAMPLE_RATES), in the subset and by the choice rule
    written above this function, at `level` 0 (fixed predictors) or 1 (LPC subframes too): a pure function of the samples, the rate and
    the level, which `ops.wave_flac` equals byte for byte.  An empty input is the 42-byte header alone, with total 0 and frame sizes 0."""
    pcm, rate, level = _as_pcm16(pcm), _flac_rate(sample_rate), check_flac_level(level)
    frames = _flac_frames(pcm, 0, FLAC_RATE_CODES[rate], level)
    sizes = [len(f) for f in frames] or [0]
    return np.frombuffer(flac_stream_header(rate, len(pcm), min(sizes), max(sizes)) + b"".join(frames), dtype=np.uint8).copy()


class StreamFlacEncoder:
    """`encode_flac` one piece at a time: `header()` is the 42 bytes with total samples 0 and frame sizes 0 (unknown length), `feed(piece)`
    the bytes of every 4096-sample frame the piece completes, `flush()` the short last frame.  The concatenation of everything `feed` and
    `flush` return equals `encode_flac(..., level)[42:]` of the concatenated input, whatever the piece sizes: a frame depends on its own
    samples and its number alone."""

    def __init__(self, sample_rate, level=0):
        self.sample_rate = _flac_rate(sample_rate)
        self.level = check_flac_level(level)
        self.code = FLAC_RATE_CODES[self.sample_rate]
        self.pending = np.zeros(0, dtype=np.int16)
        self.frames = 0

    def header(self) -> bytes:
        return flac_stream_header(self.sample_rate)

    def _emit(self, pcm):
        frames = _flac_frames(pcm, self.frames, self.code, self.level)
        self.frames += len(frames)
        return b"".join(frames)

    def feed(self, piece) -> bytes:
        self.pending = np.concatenate([self.pending, _as_pcm16(piece)])
        whole = len(self.pending) // FLAC_BLOCK * FLAC_BLOCK
        ready, self.pending = self.pending[:whole], self.pending[whole:]
        return self._emit(ready)

    def flush(self) -> bytes:
        ready, self.pending = self.pending, np.zeros(0, dtype=np.int16)
        return self._emit(ready)


class StreamDelivery:
    """`deliver_pcm16` of a `WaveSpec` one float32 piece at a time: `feed(piece)` returns the output pieces that piece releases (the piece
    through `quantise_pcm16`, a `StreamResampler`, and `encode_g711` or a `StreamFlacEncoder`; no empty ones), `finish()` the rest: the
    resampler's flush and, for FLAC, the short last frame.  Their concatenation equals `deliver_pcm16` of the quantised whole byte for byte --
    for FLAC from byte 42 on: the 42-byte header with the totals unknown comes in front of what the first piece releases, never before a
    first piece exists (a stream's first `next()` still runs the request), and from `finish()` for a stream that never had a piece."""

    def __init__(self, spec):
        self.resampler, self.encoding = StreamResampler(spec.sample_rate), spec.encoding
        self.flac = StreamFlacEncoder(spec.sample_rate, spec.flac_level) if spec.flac else None
        self.header_due = self.flac is not None

    def _header(self):
        due, self.header_due = self.header_due, False
        return [np.frombuffer(self.flac.header(), dtype=np.uint8)] if due else []

    def _encoded(self, pcm):
        if len(pcm) and self.flac is not None:
            pcm = np.frombuffer(self.flac.feed(pcm), dtype=np.uint8)   # the frames the samples complete
        elif len(pcm) and self.encoding != "pcm16":
            pcm = encode_g711(pcm, self.encoding)
        return [pcm] if len(pcm) else []

    def feed(self, piece) -> list:
        return self._header() + self._encoded(self.resampler.feed(quantise_pcm16(piece)))

    def finish(self) -> list:
        out = self._header() + self._encoded(self.resampler.flush())
        last = self.flac.flush() if self.flac is not None else b""
        return out + ([np.frombuffer(last, dtype=np.uint8)] if last else [])


class _FlacBits:
    """Big-endian bit reader over bytes: one Python integer (a read is a shift and a mask) and, for the unary parts, one byte per bit."""

    def __init__(self, data):
        self.n = 8 * len(data)
        self.v = int.from_bytes(data, "big")
        self.bits = None
        self.data = data
        self.pos = 0

    def read(self, bits):
        if self.pos + bits > self.n:
            raise ValueError("truncated FLAC stream")
        self.pos += bits
        return (self.v >> (self.n - self.pos)) & ((1 << bits) - 1)

    def signed(self, bits):
        v = self.read(bits)
        return v - (1 << bits) if bits and v >> (bits - 1) else v

    def unary(self):
        """Zero bits up to the next one bit, which is consumed."""
        if self.bits is None:
            self.bits = np.unpackbits(np.frombuffer(self.data, dtype=np.uint8)).tobytes()
        one = self.bits.find(b"\x01", self.pos)
        if one < 0:
            raise ValueError("truncated FLAC stream")
        zeros, self.pos = one - self.pos, one + 1
        return zeros


_FLAC_BLOCK_SIZES = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, **{c: 256 << (c - 8) for c in range(8, 16)}}


def _flac_residual(rd, b, o):
    method = rd.read(2)
    if method > 1:
        raise ValueError(f"unsupported FLAC stream: residual coding method {method}")
    pbits, porder = 4 + method, rd.read(4)
    if b % (1 << porder) or (b >> porder) < o:
        raise ValueError("corrupt FLAC stream: partition order does not fit the block")
    out = []
    for p in range(1 << porder):
        n = (b >> porder) - (o if p == 0 else 0)
        k = rd.read(pbits)
        if k == (1 << pbits) - 1:                                # the escape code: n raw values
            raw = rd.read(5)
            out += [rd.signed(raw) for _ in range(n)]
            continue
        for _ in range(n):
            u = (rd.unary() << k) | rd.read(k)
            out.append(u >> 1 if not u & 1 else -(u >> 1) - 1)
    return np.array(out, dtype=np.int64)


def _flac_unpredict(warm, res):
    """The samples of a fixed subframe of order len(warm): the order's differences summed back up, level by level."""
    o = len(warm)
    levels = [np.asarray(warm, dtype=np.int64)]                   # levels[j]: the j-th differences known from the warm-up, from index j on
    for _ in range(o):
        levels.append(np.diff(levels[-1]))
    seq = res
    for j in range(o - 1, -1, -1):                                # the (j+1)-th differences from index o on -> the j-th from index o on
        seq = levels[j][-1] + np.cumsum(seq)
    return np.concatenate([levels[0], seq])


def decode_flac(stream):
    """(int16 PCM, sample_rate) of a native FLAC stream: any mono 16-bit stream of CONSTANT, VERBATIM and FIXED subframes -- `encode_flac`'s
    own, and an upload's.  Both CRCs of every frame are checked.  Anything else (more channels, another sample size, an LPC subframe, a bad
    checksum, a truncated or malformed stream) raises ValueError."""
    data = bytes(stream.tobytes() if isinstance(stream, np.ndarray) else stream)
    if data[:4] != b"fLaC":
        raise ValueError(f"not a FLAC stream (starts with {data[:4]!r})")
    pos, info = 4, None
    while True:
        if pos + 4 > len(data):
            raise ValueError("truncated FLAC stream: metadata")
        kind, size = data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        last, pos = data[pos] >> 7, pos + 4
        if pos + size > len(data):
            raise ValueError("truncated FLAC stream: metadata")
        if info is None:
            if kind != 0 or size != 34:
                raise ValueError("corrupt FLAC stream: the first metadata block is not STREAMINFO")
            info = int.from_bytes(data[pos + 10:pos + 18], "big")
        pos += size
        if last:
            break
    rate, channels, bps, total = info >> 44, ((info >> 41) & 7) + 1, ((info >> 36) & 31) + 1, info & ((1 << 36) - 1)
    if channels != 1 or bps != 16:
        raise ValueError(f"unsupported FLAC stream: {channels} channel(s) at {bps} bits (mono 16-bit only)")
    blocks, count = [], 0
    while pos < len(data):
        start = pos
        rd = _FlacBits(data[pos:pos + 16])
        if rd.n < 40 or rd.read(15) != 0x7FFC:
            raise ValueError(f"corrupt FLAC stream: no frame sync at byte {pos}")
        rd.read(1)                                               # blocking strategy: the coded number is not needed to decode
        bs_code, rate_code, ch_code, size_code, reserved = rd.read(4), rd.read(4), rd.read(4), rd.read(3), rd.read(1)
        if ch_code != 0 or size_code not in (0, 4) or reserved or bs_code == 0 or rate_code == 15:
            raise ValueError("unsupported FLAC stream: a frame that is not mono 16-bit")
        lead = rd.read(8)
        extra = 0 if lead < 0x80 else 8 - (lead ^ 0xFF).bit_length() - 1 if lead >= 0xC0 and lead != 0xFF else -1
        if extra < 0:
            raise ValueError("corrupt FLAC stream: frame number")
        for _ in range(extra):
            if rd.read(8) >> 6 != 2:
                raise ValueError("corrupt FLAC stream: frame number")
        b = rd.read(8) + 1 if bs_code == 6 else rd.read(16) + 1 if bs_code == 7 else _FLAC_BLOCK_SIZES[bs_code]
        rd.read({12: 8, 13: 16, 14: 16}.get(rate_code, 0))
        hlen = rd.pos // 8
        if flac_crc8(data[pos:pos + hlen]) != rd.read(8):
            raise ValueError(f"corrupt FLAC stream: header CRC-8 of the frame at byte {start}")
        rd = _FlacBits(data[pos + hlen + 1:pos + hlen + 1 + 8 * b + 1024])   # (four times VERBATIM: no sane subframe is larger)
        if rd.read(1):
            raise ValueError("corrupt FLAC stream: subframe padding bit")
        typ, wasted = rd.read(6), rd.read(1)
        if wasted:
            wasted = rd.unary() + 1
        depth = 16 - wasted
        if depth < 1:
            raise ValueError("corrupt FLAC stream: wasted bits")
        if typ == 0:
            x = np.full(b, rd.signed(depth), dtype=np.int64)
        elif typ == 1:
            x = np.array([rd.signed(depth) for _ in range(b)], dtype=np.int64)
        elif 8 <= typ <= 12 and typ - 8 <= b:
            warm = [rd.signed(depth) for _ in range(typ - 8)]
            x = _flac_unpredict(warm, _flac_residual(rd, b, typ - 8))
        else:
            raise ValueError(f"unsupported FLAC stream: subframe type {typ:#04x} (CONSTANT, VERBATIM and FIXED only)")
        x = x << wasted
        if len(x) != b or x.min() < -32768 or x.max() > 32767:
            raise ValueError("corrupt FLAC stream: samples outside 16 bits")
        end = pos + hlen + 1 + (rd.pos + 7) // 8
        if end + 2 > len(data):
            raise ValueError("truncated FLAC stream: frame")
        if flac_crc16(data[start:end]) != int.from_bytes(data[end:end + 2], "big"):
            raise ValueError(f"corrupt FLAC stream: CRC-16 of the frame at byte {start}")
        blocks.append(x.astype(np.int16))
        count += b
        pos = end + 2
    if total and total != count:
        raise ValueError(f"corrupt FLAC stream: STREAMINFO names {total} samples, the frames hold {count}")
    return (np.concatenate(blocks) if blocks else np.zeros(0, dtype=np.int16)), int(rate)


# --- FLAC in: the whole native format (RFC 9639), defined on the host in Python integers -----------------------------------------
# `read_flac` is the definition that the device decoder (csrc/flac_in_core.h, csrc/flac_in.h, `ops.flac_decode`) equals bit for bit:
# the two accept the same streams and return the same samples.  `decode_flac` above stays the narrow reader of `encode_flac`'s subset.
FLAC_MAX_SECONDS = 600                      # audio per stream: a few bytes of CONSTANT frames can declare 2**36 samples
FLAC_DEVICE_MAX_BLOCK = 16384               # the device decoder's limits (include/f5hip.h f5hip_flac_decode): wider streams are
FLAC_DEVICE_MAX_CHANNELS = 2                # decoded by `read_flac` on the host
FLAC_DEVICE_BITS = (8, 24)
_FLAC_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_FLAC_SAMPLE_SIZES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}
_FLAC_FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))   # the fixed predictors as LPC coefficients at shift 0


def _audio_bytes(src) -> bytes:
    if isinstance(src, np.ndarray):
        return src.tobytes()
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    if hasattr(src, "read"):
        return src.read()
    with open(os.fspath(src), "rb") as f:
        return f.read()


def flac_stream_info(data):
    """The STREAMINFO fields of a native FLAC stream and where its frames begin, as a dict (min_block, max_block, rate, channels, bits,
    total, md5, first: the byte after the last metadata block).  Refuses (ValueError) what needs no samples to refuse: the magic, the
    metadata chain, a sample size under 4 bits, rate 0, and a declared total beyond FLAC_MAX_SECONDS."""
    if data[:4] != b"fLaC":
        raise ValueError(f"not a FLAC stream (starts with {bytes(data[:4])!r})")
    pos, info = 4, None
    while True:
        if pos + 4 > len(data):
            raise ValueError("truncated FLAC stream: metadata")
        kind, size = data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        last, pos = data[pos] >> 7, pos + 4
        if pos + size > len(data):
            raise ValueError("truncated FLAC stream: metadata")
        if info is None:
            if kind != 0 or size != 34:
                raise ValueError("corrupt FLAC stream: the first metadata block is not STREAMINFO")
            info = data[pos:pos + 34]
        pos += size
        if last:
            break
    word = int.from_bytes(info[10:18], "big")
    out = dict(min_block=int.from_bytes(info[0:2], "big"), max_block=int.from_bytes(info[2:4], "big"), rate=word >> 44,
               channels=((word >> 41) & 7) + 1, bits=((word >> 36) & 31) + 1, total=word & ((1 << 36) - 1), md5=bytes(info[18:34]), first=pos)
    if out["bits"] < 4:
        raise ValueError(f"corrupt FLAC stream: STREAMINFO names {out['bits']} bits per sample")
    if out["rate"] == 0:
        raise ValueError("unsupported FLAC stream: sample rate 0")
    if out["total"] > FLAC_MAX_SECONDS * out["rate"]:
        raise ValueError(f"FLAC stream too long: STREAMINFO names {out['total']} samples at {out['rate']} Hz (at most {FLAC_MAX_SECONDS} s)")
    return out


def flac_needs_host(info) -> bool:
    """Whether a stream (its `flac_stream_info`) lies outside the device decoder's limits."""
    return info["channels"] > FLAC_DEVICE_MAX_CHANNELS or not FLAC_DEVICE_BITS[0] <= info["bits"] <= FLAC_DEVICE_BITS[1]


def flac_check_md5(samples, info):
    """The last check of a decoded stream, on the host for both decoders: STREAMINFO's MD5, when non-zero, against the interleaved
    little-endian samples at ceil(bits / 8) bytes each."""
    if info["md5"] == bytes(16):
        return
    width = (info["bits"] + 7) // 8
    raw = np.ascontiguousarray(samples.T).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :width]
    found = hashlib.md5(raw.tobytes()).digest()
    if found != info["md5"]:
        raise ValueError(f"corrupt FLAC stream: STREAMINFO's MD5 is {info['md5'].hex()}, the samples' {found.hex()}")


def _flac_frame_header(data, pos, info):
    """The header of the frame at byte `pos`: dict(variable, block, rate, code (the channel code), channels, bits, number, size: its
    bytes, the CRC-8 included)."""
    rd = _FlacBits(data[pos:pos + 16])
    if rd.read(14) != 0x3FFE:
        raise ValueError(f"corrupt FLAC stream: no frame sync at byte {pos}")
    if rd.read(1):
        raise ValueError(f"corrupt FLAC stream: reserved bit after the sync of the frame at byte {pos}")
    variable = rd.read(1)
    bs_code, rate_code, ch_code, size_code = rd.read(4), rd.read(4), rd.read(4), rd.read(3)
    if bs_code == 0:
        raise ValueError(f"corrupt FLAC stream: reserved block-size code 0 in the frame at byte {pos}")
    if rate_code == 15:
        raise ValueError(f"corrupt FLAC stream: invalid sample-rate code 15 in the frame at byte {pos}")
    if ch_code > 10:
        raise ValueError(f"corrupt FLAC stream: reserved channel code {ch_code} in the frame at byte {pos}")
    if size_code == 3:
        raise ValueError(f"corrupt FLAC stream: reserved sample-size code 3 in the frame at byte {pos}")
    if rd.read(1):
        raise ValueError(f"corrupt FLAC stream: reserved bit in the header of the frame at byte {pos}")
    lead = rd.read(8)
    extra = 0 if lead < 0x80 else 7 - (lead ^ 0xFF).bit_length() if 0xC0 <= lead <= (0xFE if variable else 0xFC) else -1
    if extra < 0:
        raise ValueError(f"corrupt FLAC stream: coded number of the frame at byte {pos} (lead byte {lead:#04x})")
    number = lead if not extra else lead & (0x7F >> (extra + 1))
    for _ in range(extra):
        c = rd.read(8)
        if c >> 6 != 2:
            raise ValueError(f"corrupt FLAC stream: coded number of the frame at byte {pos} (continuation byte {c:#04x})")
        number = (number << 6) | (c & 0x3F)
    block = rd.read(8) + 1 if bs_code == 6 else rd.read(16) + 1 if bs_code == 7 else _FLAC_BLOCK_SIZES[bs_code]
    if block > 65535:
        raise ValueError(f"corrupt FLAC stream: block size {block} in the frame at byte {pos}")
    rate = (info["rate"] if rate_code == 0 else rd.read(8) * 1000 if rate_code == 12 else rd.read(16) if rate_code == 13
            else rd.read(16) * 10 if rate_code == 14 else _FLAC_RATES[rate_code])
    size = rd.pos // 8
    if flac_crc8(data[pos:pos + size]) != rd.read(8):
        raise ValueError(f"corrupt FLAC stream: header CRC-8 of the frame at byte {pos}")
    return dict(variable=variable, block=block, rate=rate, code=ch_code, channels=ch_code + 1 if ch_code < 8 else 2,
                bits=_FLAC_SAMPLE_SIZES[size_code] if size_code else info["bits"], number=number, size=size + 1)


def _flac_restore(warm, res, coefs, shift, depth):
    """warm-up + residuals -> samples by `s[i] = res[i] + (sum(coefs[j] * s[i-1-j]) >> shift)`, in Python integers; stops with ValueError
    at the first sample outside `depth` bits, so no later value is ever built on one."""
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    s = [int(v) for v in warm]
    for v in s:
        if not lo <= v <= hi:                                    # (only a 1-bit depth's warm-up can be here: signed(depth) is in range)
            raise ValueError(f"corrupt FLAC stream: samples outside {depth} bits")
    o = len(coefs)
    rev = tuple(reversed(coefs))                                 # rev[j] multiplies s[i - o + j]
    for i, r in enumerate(res.tolist(), o):
        acc = 0
        for c, v in zip(rev, s[i - o:i]):
            acc += c * v
        v = r + (acc >> shift)
        if not lo <= v <= hi:
            raise ValueError(f"corrupt FLAC stream: samples outside {depth} bits")
        s.append(v)
    return s


def _flac_subframe(rd, b, depth):
    """One subframe of `b` samples at `depth` bits, from the bit reader: a list of Python integers."""
    if rd.read(1):
        raise ValueError("corrupt FLAC stream: subframe padding bit")
    typ, wasted = rd.read(6), rd.read(1)
    if wasted:
        wasted = rd.unary() + 1
    depth -= wasted
    if depth < 1:
        raise ValueError(f"corrupt FLAC stream: {wasted} wasted bits leave no sample bits")
    if typ == 0:
        x = [rd.signed(depth)] * b
    elif typ == 1:
        x = [rd.signed(depth) for _ in range(b)]
    elif 8 <= typ <= 12 or typ >= 32:
        o = typ - 8 if typ < 32 else typ - 31
        if o > b:
            raise ValueError(f"corrupt FLAC stream: predictor order {o} in a block of {b}")
        warm = [rd.signed(depth) for _ in range(o)]
        if typ < 32:
            coefs, shift = _FLAC_FIXED[o], 0
        else:
            precision = rd.read(4) + 1
            if precision == 16:
                raise ValueError("corrupt FLAC stream: invalid LPC precision code 1111")
            shift = rd.signed(5)
            if shift < 0:
                raise ValueError(f"corrupt FLAC stream: negative LPC shift {shift}")
            coefs = tuple(rd.signed(precision) for _ in range(o))
        res = _flac_residual(rd, b, o)
        if len(res) and (res.min() < -(1 << 31) or res.max() >= 1 << 31):
            raise ValueError("corrupt FLAC stream: a residual outside 32 bits")
        x = _flac_restore(warm, res, coefs, shift, depth)
    else:
        raise ValueError(f"corrupt FLAC stream: reserved subframe type {typ:#04x}")
    return [v << wasted for v in x] if wasted else x


def _flac_frame_body(data, start, hdr, info):
    """The subframes and CRC-16 of the frame at `start`: (channel lists before stereo reconstruction, the frame's end).  The bit reader
    takes a window of the stream and the parse is repeated on a larger one if it runs out, so reads are bounded by the stream alone."""
    b, body = hdr["block"], start + hdr["size"]
    window = hdr["channels"] * (b * hdr["bits"] // 8 + 64) + 1024
    while True:
        rd = _FlacBits(data[body:body + window])
        try:
            chans = []
            for c in range(hdr["channels"]):
                side = (hdr["code"] in (8, 10) and c == 1) or (hdr["code"] == 9 and c == 0)
                chans.append(_flac_subframe(rd, b, hdr["bits"] + side))
            end = body + (rd.pos + 7) // 8
            if end + 2 > len(data):
                raise ValueError("truncated FLAC stream: frame")
            break
        except ValueError as e:
            if not str(e).startswith("truncated") or body + window >= len(data):
                raise
            window *= 4
    if flac_crc16(data[start:end]) != int.from_bytes(data[end:end + 2], "big"):
        raise ValueError(f"corrupt FLAC stream: CRC-16 of the frame at byte {start}")
    return chans, end + 2


def flac_unstereo(code, a, b):
    """Channel planes (int64 arrays) of a two-channel frame from its coded pair: 8 left/side, 9 side/right, 10 mid/side."""
    if code == 8:
        return a, a - b
    if code == 9:
        return a + b, b
    if code == 10:
        m = (a << 1) | (b & 1)
        return (m + b) >> 1, (m - b) >> 1
    return a, b


def read_flac(stream):
    """(samples int32 [channels, n], sample_rate, bits) of a native FLAC stream (RFC 9639): every subframe type, LPC order, Rice method,
    stereo mode, bit depth, channel count and blocking strategy.  Checked, each a ValueError naming what was found: both CRCs of every
    frame, every reserved code, frame / sample numbers in sequence, block sizes, sample size, rate and channel count against STREAMINFO,
    samples inside their bit depth, residuals inside 32 bits, STREAMINFO's total and MD5 when non-zero, and FLAC_MAX_SECONDS of audio
    (against STREAMINFO before decoding, against the running count while decoding).  Serial Python: seconds per clip; `ops.flac_decode`
    is the same function on the device."""
    data = _audio_bytes(stream)
    info = flac_stream_info(data)
    pos, count, index, first, planes = info["first"], 0, 0, None, []
    cap = FLAC_MAX_SECONDS * info["rate"]
    lo, hi = -(1 << (info["bits"] - 1)), (1 << (info["bits"] - 1)) - 1
    while pos < len(data):
        try:
            hdr = _flac_frame_header(data, pos, info)
        except ValueError as e:
            if str(e).startswith("truncated"):
                raise ValueError(f"truncated FLAC stream: header of the frame at byte {pos}") from None
            raise
        b = hdr["block"]
        if (hdr["channels"], hdr["bits"], hdr["rate"]) != (info["channels"], info["bits"], info["rate"]):
            raise ValueError(f"unsupported FLAC stream: the frame at byte {pos} has {hdr['channels']} channel(s) at {hdr['bits']} bits and "
                             f"{hdr['rate']} Hz, STREAMINFO {info['channels']} at {info['bits']} and {info['rate']}")
        if first is None:
            first = hdr
        if hdr["variable"] != first["variable"]:
            raise ValueError(f"corrupt FLAC stream: the blocking strategy changes at byte {pos}")
        if hdr["number"] != (count if hdr["variable"] else index):
            raise ValueError(f"corrupt FLAC stream: the frame at byte {pos} is numbered {hdr['number']}, "
                             f"expected {count if hdr['variable'] else index}")
        if info["max_block"] and b > info["max_block"]:
            raise ValueError(f"corrupt FLAC stream: block of {b} at byte {pos}, STREAMINFO's largest is {info['max_block']}")
        if count + b > cap:
            raise ValueError(f"FLAC stream too long: more than {FLAC_MAX_SECONDS} s at {info['rate']} Hz")
        chans, end = _flac_frame_body(data, pos, hdr, info)
        if end < len(data):                                       # not the last frame, which alone may be short
            if b < info["min_block"]:
                raise ValueError(f"corrupt FLAC stream: block of {b} at byte {pos}, STREAMINFO's smallest is {info['min_block']}")
            if not hdr["variable"] and b != first["block"]:
                raise ValueError(f"corrupt FLAC stream: block of {b} at byte {pos} in a fixed-blocking stream of {first['block']}")
        x = np.array(chans, dtype=np.int64)
        if hdr["code"] >= 8:
            x = np.stack(flac_unstereo(hdr["code"], x[0], x[1]))
            if x.min() < lo or x.max() > hi:
                raise ValueError(f"corrupt FLAC stream: samples outside {info['bits']} bits")
        planes.append(x.astype(np.int32))
        count, index, pos = count + b, index + 1, end
    samples = np.concatenate(planes, axis=1) if planes else np.zeros((info["channels"], 0), dtype=np.int32)
    if info["total"] and info["total"] != count:
        raise ValueError(f"corrupt FLAC stream: STREAMINFO names {info['total']} samples, the frames hold {count}")
    flac_check_md5(samples, info)
    return samples, int(info["rate"]), int(info["bits"])


def is_flac(data) -> bool:
    """The sniffing rule of `load_audio`: "fLaC" followed by a STREAMINFO block header (type 0, last or not, length 34)."""
    return len(data) >= 8 and bytes(data[:4]) == b"fLaC" and data[4] & 0x7F == 0 and bytes(data[5:8]) == b"\x00\x00\x22"


def load_audio(src, flac=None):
    """`load_wav` that also takes native FLAC: a source that starts with "fLaC" and a STREAMINFO block header goes to `flac` (default
    `read_flac`; the server passes the device decoder) and is scaled like PCM in a WAV file, / 2**(bits - 1), exact in float32 up to 24
    bits; everything else goes to `load_wav` unchanged, its refusals included."""
    data = _audio_bytes(src)
    if not is_flac(data):
        return load_wav(data)
    samples, rate, bits = (flac or read_flac)(data)
    x = torch.from_numpy(np.ascontiguousarray(samples).astype(np.float64) / float(1 << (bits - 1))).to(torch.float32)
    return x, rate
