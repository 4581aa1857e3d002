"""Reference-audio pre-step of the reference's inference driver, restated without pydub.

Mirrors `preprocess_ref_audio_text` / `remove_silence_edges` (F/infer/utils_infer.py:263-350): clip a long reference
clip at a pause (>= 1 s below -50 dBFS, else >= 0.1 s below -40 dBFS, else a hard cut at 15 s), strip leading / trailing
silence (-42 dBFS), append 50 ms of silence, write a temporary 16-bit WAV, and normalise the end of the reference text
(". " rule).  Returns `(wav_path, ref_text)` like the reference, so `infer_process(*preprocess_ref_audio_text(...), ...)`
reads the same.

pydub (0.25.1) is a third-party dependency that is absent here; its published algorithms are restated on int16 numpy
arrays: millisecond slicing (`frame = int(ms * rate / 1000)`), `rms` = floor(sqrt(mean(x^2))) over all interleaved samples
(audioop.rms), `dBFS` = 20 log10(rms / 32768), `silence.detect_silence` / `detect_nonsilent` / `split_on_silence` /
`detect_leading_silence`.  PARITY UNPINNED by the reference (no fixture of it exists); pinned by known-answer tests on
synthetic tone / pause signals and against the stdlib `audioop.rms` (tests/test_host_glue.py).  Differences, explicit:
  * input is a 16-bit PCM WAV (stdlib `wave`); pydub would hand other containers to ffmpeg;
  * sample rates below 11 025 Hz are rejected (pydub would up-sample them to its 11 025 Hz "silent" segment's rate);
  * an empty `ref_text` raises: the reference transcribes with a Whisper pipeline that is not part of this path.
"""
from __future__ import annotations

import hashlib
import math
import tempfile
import typing
import wave as _wave

import numpy as np

from . import wave_codec

_MAX_AMP = 32768.0   # AudioSegment.max_possible_amplitude for 16-bit samples


class PcmSegment:
    """The subset of pydub.AudioSegment the pre-step uses: int16 frames [n, channels] at `rate`, sliced in milliseconds."""

    def __init__(self, frames: np.ndarray, rate: int):
        frames = np.asarray(frames, dtype=np.int16)
        self.frames = frames.reshape(-1, 1) if frames.ndim == 1 else frames
        self.rate = int(rate)
        self._csq = None

    @classmethod
    def from_wav(cls, path: str) -> "PcmSegment":
        with open(path, "rb") as f:
            head = f.read(8)
        if wave_codec.is_flac(head):                                  # a FLAC voice file: any depth, quantised by the routes' rule
            wav, rate = wave_codec.load_audio(path)
            return cls(wave_codec.quantise_pcm16(wav.numpy().T), rate)
        with _wave.open(path, "rb") as f:
            rate, ch, sw, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
            raw = f.readframes(n)
        if sw != 2:
            raise ValueError("only 16-bit PCM WAV reference audio is supported")
        return cls(np.frombuffer(raw, dtype="<i2").reshape(-1, ch), rate)

    @classmethod
    def silent(cls, duration_ms: int, rate: int, channels: int = 1) -> "PcmSegment":
        return cls(np.zeros((int(rate * duration_ms / 1000.0), channels), dtype=np.int16), rate)

    def __len__(self) -> int:                      # pydub: round(1000 * frame_count / frame_rate)
        return int(round(1000.0 * self.frames.shape[0] / self.rate))

    def _frame(self, ms) -> int:                   # pydub _parse_position: int(ms * frame_rate / 1000.0), clipped
        return min(max(int(ms * (self.rate / 1000.0)), 0), self.frames.shape[0])

    def slice_ms(self, start_ms, end_ms) -> "PcmSegment":
        start_ms = max(0, min(start_ms, len(self)))
        end_ms = max(0, min(end_ms, len(self)))
        return PcmSegment(self.frames[self._frame(start_ms):self._frame(end_ms)], self.rate)

    def __add__(self, other: "PcmSegment") -> "PcmSegment":
        if other.rate != self.rate or other.frames.shape[1] != self.frames.shape[1]:
            raise ValueError("segments must share rate and channel count")
        return PcmSegment(np.concatenate([self.frames, other.frames]), self.rate)

    def _cum_squares(self) -> np.ndarray:          # exact in int64: 2^30 per sample
        if self._csq is None:
            sq = self.frames.astype(np.int64)
            np.multiply(sq, sq, out=sq)
            sq = sq[:, 0] if sq.shape[1] == 1 else sq.sum(axis=1)
            csq = np.zeros(len(sq) + 1, dtype=np.int64)
            np.cumsum(sq, out=csq[1:])
            self._csq = csq
        return self._csq

    def rms_ms(self, start_ms, end_ms) -> int:
        """audioop.rms of the millisecond window: floor(sqrt(sum x^2 / n_samples)) over all interleaved samples."""
        a, b = self._frame(max(0, min(start_ms, len(self)))), self._frame(max(0, min(end_ms, len(self))))
        n = (b - a) * self.frames.shape[1]
        if n <= 0:
            return 0
        c = self._cum_squares()
        return int(math.sqrt(float(c[b] - c[a]) / n))

    def _frames(self, ms: np.ndarray) -> np.ndarray:
        """`_frame` of every entry of an integer millisecond array (the same float product, truncated, clipped)."""
        return np.clip((ms * (self.rate / 1000.0)).astype(np.int64), 0, self.frames.shape[0])

    def rms_windows(self, start_ms: np.ndarray, end_ms: np.ndarray) -> np.ndarray:
        """`rms_ms(start_ms[i], end_ms[i])` for every i at once, as int64: the sums are differences of the exact int64 cumulative squares,
        then the same float conversion, division, square root and truncation as `rms_ms`."""
        n_ms = len(self)
        a = self._frames(np.clip(np.asarray(start_ms, dtype=np.int64), 0, n_ms))
        b = self._frames(np.clip(np.asarray(end_ms, dtype=np.int64), 0, n_ms))
        n = (b - a) * self.frames.shape[1]
        c = self._cum_squares()
        out = np.zeros(a.shape, dtype=np.int64)
        ok = n > 0
        out[ok] = np.sqrt((c[b[ok]] - c[a[ok]]).astype(np.float64) / n[ok]).astype(np.int64)
        return out

    @property
    def rms(self) -> int:
        return self.rms_ms(0, len(self) + 1)

    def dbfs_ms(self, start_ms, end_ms) -> float:
        r = self.rms_ms(start_ms, end_ms)
        return -math.inf if r == 0 else 20.0 * math.log10(r / _MAX_AMP)

    @property
    def duration_seconds(self) -> float:
        return self.frames.shape[0] / self.rate

    def export_wav(self, path: str) -> None:
        with _wave.open(path, "wb") as f:
            f.setnchannels(self.frames.shape[1]); f.setsampwidth(2); f.setframerate(self.rate)
            f.writeframes(np.ascontiguousarray(self.frames, dtype="<i2").tobytes())


def detect_silence(seg: PcmSegment, min_silence_len=1000, silence_thresh=-16, seek_step=1):
    """pydub.silence.detect_silence: [start_ms, end_ms] ranges whose every `min_silence_len` window has rms <= threshold.
    All windows are measured in one pass over the cumulative squares (`rms_windows`)."""
    seg_len = len(seg)
    if seg_len < min_silence_len:
        return []
    thresh = (10 ** (silence_thresh / 20.0)) * _MAX_AMP
    last = seg_len - min_silence_len
    starts = np.arange(0, last + 1, seek_step, dtype=np.int64)
    if last % seek_step:
        starts = np.append(starts, last)
    silent = starts[seg.rms_windows(starts, starts + min_silence_len) <= thresh]
    if not len(silent):
        return []
    # a new range starts at a silent window that neither continues the previous one nor begins inside it
    cut = np.flatnonzero((silent[1:] != silent[:-1] + seek_step) & (silent[1:] > silent[:-1] + min_silence_len))
    first = np.concatenate([silent[:1], silent[cut + 1]])
    end = np.concatenate([silent[cut], silent[-1:]]) + min_silence_len
    return [[int(a), int(b)] for a, b in zip(first, end)]


def detect_nonsilent(seg: PcmSegment, min_silence_len=1000, silence_thresh=-16, seek_step=1):
    silent = detect_silence(seg, min_silence_len, silence_thresh, seek_step)
    n = len(seg)
    if not silent:
        return [[0, n]]
    if silent[0][0] == 0 and silent[0][1] == n:
        return []
    out, prev_end, end = [], 0, 0
    for start, end in silent:
        out.append([prev_end, start])
        prev_end = end
    if end != n:
        out.append([prev_end, n])
    if out[0] == [0, 0]:
        out.pop(0)
    return out


def split_on_silence(seg: PcmSegment, min_silence_len=1000, silence_thresh=-16, keep_silence=100, seek_step=1):
    """pydub.silence.split_on_silence (0.25.1): non-silent chunks padded by `keep_silence` ms, overlaps split at the midpoint."""
    ranges = [[s - keep_silence, e + keep_silence] for s, e in detect_nonsilent(seg, min_silence_len, silence_thresh, seek_step)]
    for a, b in zip(ranges, ranges[1:]):
        if b[0] < a[1]:
            a[1] = (a[1] + b[0]) // 2
            b[0] = a[1]
    return [seg.slice_ms(max(s, 0), min(e, len(seg))) for s, e in ranges]


def _dbfs_of_rms(r: int) -> float:
    return -math.inf if r == 0 else 20.0 * math.log10(r / _MAX_AMP)


def _where_dbfs(rms: np.ndarray, pred) -> np.ndarray:
    """pred(dBFS) of every window rms, the dBFS worked out by the scalar rule once per distinct rms value."""
    values, inverse = np.unique(rms, return_inverse=True)
    return np.array([bool(pred(_dbfs_of_rms(int(v)))) for v in values], dtype=bool)[inverse]


def detect_leading_silence(seg: PcmSegment, silence_threshold=-50.0, chunk_size=10) -> int:
    n_ms = len(seg)
    trims = np.arange(0, n_ms, chunk_size, dtype=np.int64)        # the positions the reference's loop can stop at before the end
    loud = ~_where_dbfs(seg.rms_windows(trims, trims + chunk_size), lambda db: db < silence_threshold)
    hit = np.flatnonzero(loud)
    return int(trims[hit[0]]) if len(hit) else n_ms


def remove_silence_edges(seg: PcmSegment, silence_threshold=-42) -> PcmSegment:
    """F/infer/utils_infer.py:263-277: leading silence in 10 ms chunks, trailing silence one millisecond at a time."""
    seg = seg.slice_ms(detect_leading_silence(seg, silence_threshold), len(seg) + 1)
    end = seg.duration_seconds
    ms = np.arange(len(seg), dtype=np.int64)
    loud = np.flatnonzero(_where_dbfs(seg.rms_windows(ms, ms + 1), lambda db: db > silence_threshold))
    quiet_tail = len(seg) - 1 - int(loud[-1]) if len(loud) else len(seg)
    for _ in range(quiet_tail):       # the reference's own running subtraction, rounding included
        end -= 0.001
    return seg.slice_ms(0, int(end * 1000))


def _clip_at_pause(seg: PcmSegment, min_silence_len: int, silence_thresh: int, show_info, tag: str) -> PcmSegment:
    out = PcmSegment(np.zeros((0, seg.frames.shape[1]), dtype=np.int16), seg.rate)
    for chunk in split_on_silence(seg, min_silence_len=min_silence_len, silence_thresh=silence_thresh, keep_silence=1000, seek_step=10):
        if len(out) > 6000 and len(out + chunk) > 15000:
            show_info(f"Audio is over 15s, clipping short. ({tag})")
            break
        out = out + chunk
    return out


_ref_text_cache: dict = {}   # audio md5 -> transcription (the reference caches ASR output only; kept for interface parity)


def preprocess_ref_segment(seg: PcmSegment, clip_short: bool = True, show_info=print) -> PcmSegment:
    """The audio part of F/infer/utils_infer.py:282-350 between reading the clip and writing the temporary WAV: clip at a pause
    (`clip_short`), strip the silent edges, append 50 ms of silence."""
    if seg.rate < 11025:
        raise ValueError("reference audio below 11025 Hz is not supported on this path")
    if clip_short:
        clipped = _clip_at_pause(seg, 1000, -50, show_info, "1")
        if len(clipped) > 15000:
            clipped = _clip_at_pause(seg, 100, -40, show_info, "2")
        seg = clipped
        if len(seg) > 15000:
            seg = seg.slice_ms(0, 15000)
            show_info("Audio is over 15s, clipping short. (3)")
    return remove_silence_edges(seg) + PcmSegment.silent(50, seg.rate, seg.frames.shape[1])


# ---------------------------------------------------------------------------------------------- the pre-step as ranges
# `preprocess_ref_ranges` restates `preprocess_ref_segment` as index arithmetic on the SOURCE frames: what the device call mirrors
# (csrc/ref_prestep_core.h, csrc/ref_prestep.h, `ops.ref_prestep`).  `preprocess_ref_segment` stays the definition.
#
# Every rms comparison is made on integers.  A window of n samples with the exact integer sum of squares S has rms = floor(sqrt(S / n)) in
# fp64 (`rms_ms`), and for an integer r
#     floor(sqrt(S / n)) >= r   <=>   S >= r^2 n.
# Why this is exact for the sums that can occur (r <= 328, n < 2^23 samples per window, i.e. rate x channels < 2^23):
#   * S <= 2^30 n < 2^53, so S and n are exact in fp64, and S / n and its square root are single, correctly rounded operations, both
#     monotone, with r^2 and r representable: S >= r^2 n gives S / n >= r^2, a quotient that rounds to at least r^2 and a root of at least r;
#   * S < r^2 n gives S / n <= r^2 - 1 / n with 1 / n > 2^-23, while the fp64 spacing below r^2 <= 2^17 is 2^-36 or finer: the rounded
#     quotient stays 2^-24 or more below r^2, its root 2^-24 / (2 r) >= 2^-34 or more below r, and the spacing below r < 2^9 is 2^-44:
#     no integer square (and no integer) lies within reach of either rounding.
# `rms <= thresh` of detect_silence is rms <= T with T = floor(thresh), i.e. S < (T + 1)^2 n: the form wave_silence_kernel uses.  The two
# dBFS comparisons of the edge trim become rms < r and rms >= r for integer thresholds found by evaluating `_dbfs_of_rms` itself, which is
# monotone in the integer rms.  fp64 remains only in the frame of a millisecond (`_frame`), the length in milliseconds (`__len__`) and the
# running subtraction of the trailing trim: each a single IEEE operation here and on the device.
REF_CLIP_PASSES = ((1000, -50), (100, -40))      # (min_silence_len ms, silence_thresh dBFS), tried in turn
REF_KEEP_MS, REF_SEEK_MS, REF_MIN_MS, REF_MAX_MS, REF_EDGE_DBFS, REF_TAIL_MS = 1000, 10, 6000, 15000, -42, 50


def silence_square(silence_thresh) -> int:
    """(T + 1)^2 for T = floor of detect_silence's amplitude threshold: a window is silent iff S < silence_square * n."""
    return (math.floor((10 ** (silence_thresh / 20.0)) * _MAX_AMP) + 1) ** 2


def edge_rms_thresholds(silence_threshold=REF_EDGE_DBFS):
    """(lead, trail): `dBFS(rms) < threshold` (leading silence) is rms < lead, `dBFS(rms) > threshold` (a loud trailing millisecond) is
    rms >= trail, by the scalar rule itself evaluated from rms 0 upwards."""
    lead = next(r for r in range(int(_MAX_AMP) + 2) if not _dbfs_of_rms(r) < silence_threshold)
    trail = next(r for r in range(int(_MAX_AMP) + 2) if _dbfs_of_rms(r) > silence_threshold)
    return lead, trail


def _len_ms(frames: int, rate: int) -> int:
    return int(round(1000.0 * frames / rate))


class _ClipWalk:
    """The sequential part of one `_clip_at_pause` pass over the silent window starts, with O(1) state: silent ranges -> non-silent
    ranges -> padded chunks with midpoint splits -> the 6 s / 15 s stop -> frame ranges of the source (adjacent ones merged)."""

    def __init__(self, n_frames, rate, msl):
        self.N, self.rate, self.k, self.msl = n_frames, rate, rate / 1000.0, msl
        self.L = _len_ms(n_frames, rate)
        self.have_prev = self.first = self.pend = self.stopped = False
        self.any_silent = False
        self.first = True
        self.prev = self.cur = self.prev_end = self.last_end = self.ps = self.pe = 0
        self.ranges, self.frames = [], 0

    def _frame(self, ms):
        return min(max(int(ms * self.k), 0), self.N)

    def silent_start(self, s):
        if not self.have_prev:
            self.cur = s
        elif s != self.prev + REF_SEEK_MS and s > self.prev + self.msl:
            self._silent_range(self.cur, self.prev + self.msl)
            self.cur = s
        self.prev, self.have_prev = s, True

    def _silent_range(self, s, e):
        self.any_silent = True
        self._nonsilent(self.prev_end, s, True)
        self.prev_end = self.last_end = e

    def _nonsilent(self, p, s, droppable):
        head = self.first and droppable and p == 0 and s == 0       # detect_nonsilent drops a leading [0, 0]
        self.first = False
        if head:
            return
        ns, ne = p - REF_KEEP_MS, s + REF_KEEP_MS
        if self.pend:
            if ns < self.pe:
                self.pe = (self.pe + ns) // 2
                ns = self.pe
            self._chunk(max(self.ps, 0), min(self.pe, self.L))
        self.ps, self.pe, self.pend = ns, ne, True

    def _chunk(self, a_ms, b_ms):
        if self.stopped:
            return
        fa, fb = self._frame(max(0, min(a_ms, self.L))), self._frame(max(0, min(b_ms, self.L)))
        n = max(fb - fa, 0)
        if _len_ms(self.frames, self.rate) > REF_MIN_MS and _len_ms(self.frames + n, self.rate) > REF_MAX_MS:
            self.stopped = True
            return
        if n:
            if self.ranges and self.ranges[-1][1] == fa:
                self.ranges[-1][1] = fb
            else:
                self.ranges.append([fa, fb])
            self.frames += n

    def finish(self):
        if self.have_prev:
            self._silent_range(self.cur, self.prev + self.msl)
        if not self.any_silent:
            self._nonsilent(0, self.L, False)
        elif self.last_end != self.L:
            self._nonsilent(self.prev_end, self.L, True)
        if self.pend:
            self._chunk(max(self.ps, 0), min(self.pe, self.L))
        return self.ranges, self.frames


def _silent_starts(seg: PcmSegment, msl: int, square: int) -> np.ndarray:
    """The window starts of detect_silence(seek_step 10) that are silent, by the integer comparison."""
    L = len(seg)
    if L < msl:
        return np.zeros(0, dtype=np.int64)
    last = L - msl
    starts = np.arange(0, last + 1, REF_SEEK_MS, dtype=np.int64)
    if last % REF_SEEK_MS:
        starts = np.append(starts, last)
    a, b = seg._frames(starts), seg._frames(starts + msl)
    c = seg._cum_squares()
    n = (b - a) * seg.frames.shape[1]
    return starts[(n <= 0) | (c[b] - c[a] < square * n)]


def _truncate(ranges, frames):
    out, left = [], frames
    for a, b in ranges:
        if left <= 0:
            break
        b = min(b, a + left)
        out.append([a, b])
        left -= b - a
    return out


def preprocess_ref_ranges(seg: PcmSegment, clip_short: bool = True):
    """`preprocess_ref_segment` as ranges: (ranges, tail_frames), the [a, b) frame ranges of `seg` whose frames, in order and followed by
    `tail_frames` zero frames, are the frames of preprocess_ref_segment(seg, clip_short)."""
    if seg.rate < 11025:
        raise ValueError("reference audio below 11025 Hz is not supported on this path")
    rate, N, C, k = seg.rate, seg.frames.shape[0], seg.frames.shape[1], seg.rate / 1000.0
    ranges, total = ([[0, N]] if N else []), N
    if clip_short:
        for msl, db in REF_CLIP_PASSES:
            walk = _ClipWalk(N, rate, msl)
            for s in _silent_starts(seg, msl, silence_square(db)):
                walk.silent_start(int(s))
            ranges, total = walk.finish()
            if _len_ms(total, rate) <= REF_MAX_MS:
                break
        if _len_ms(total, rate) > REF_MAX_MS:                        # slice_ms(0, 15000) of the concatenation
            total = min(int(REF_MAX_MS * k), total)
            ranges = _truncate(ranges, total)
    # remove_silence_edges on the concatenation: its millisecond grid starts at its own frame 0
    src = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in ranges]) if ranges else np.zeros(0, dtype=np.int64)
    sq = np.diff(seg._cum_squares())[src]
    csq = np.concatenate([[0], np.cumsum(sq)]).astype(np.int64)
    lead_r, trail_r = edge_rms_thresholds()

    def grid(ms, n_ms, n_frames):                                     # `_frames` of a segment of n_frames
        return np.clip((np.clip(ms, 0, n_ms) * k).astype(np.int64), 0, n_frames)

    L1 = _len_ms(total, rate)
    trims = np.arange(0, L1, REF_SEEK_MS, dtype=np.int64)
    a, b = grid(trims, L1, total), grid(trims + REF_SEEK_MS, L1, total)
    n = (b - a) * C
    loud = np.flatnonzero((n > 0) & (csq[b] - csq[a] >= lead_r * lead_r * n))
    lead = int(trims[loud[0]]) if len(loud) else L1
    x0 = int(grid(np.int64(lead), L1, total))
    n2 = int(grid(np.int64(L1), L1, total)) - x0                      # slice_ms(lead, L1 + 1)
    L2 = _len_ms(n2, rate)
    end = n2 / rate
    ms = np.arange(L2, dtype=np.int64)
    a, b = x0 + grid(ms, L2, n2), x0 + grid(ms + 1, L2, n2)
    n = (b - a) * C
    loud = np.flatnonzero((n > 0) & (csq[b] - csq[a] >= trail_r * trail_r * n))
    quiet_tail = L2 - 1 - int(loud[-1]) if len(loud) else L2
    for _ in range(quiet_tail):                                       # the reference's own running subtraction, rounding included
        end -= 0.001
    x1 = x0 + int(grid(np.int64(int(end * 1000)), L2, n2))
    out, at = [], 0
    for a, b in ranges:                                               # concatenation frames [x0, x1) back to source frames
        lo, hi = max(a, a + x0 - at), min(b, a + x1 - at)
        if lo < hi:
            out.append([int(lo), int(hi)])
        at += b - a
    return out, int(rate * REF_TAIL_MS / 1000.0)


def normalize_ref_text(ref_text: str) -> str:
    """The ". " rule at the end of the reference text (F/infer/utils_infer.py:343-348)."""
    if not ref_text.endswith(". ") and not ref_text.endswith("。"):
        ref_text += " " if ref_text.endswith(".") else ". "
    return ref_text


def preprocess_ref_audio_text(ref_audio_orig: str, ref_text: str, clip_short: bool = True, show_info=print, device=None):
    """F/infer/utils_infer.py:282-350.  Returns (path of the processed temporary WAV, normalised ref_text)."""
    seg = preprocess_ref_segment(PcmSegment.from_wav(ref_audio_orig), clip_short, show_info)
    with tempfile.NamedTemporaryFile(delete=False, suffix=".wav") as f:
        path = f.name
    seg.export_wav(path)
    with open(path, "rb") as f:
        audio_hash = hashlib.md5(f.read()).hexdigest()
    if not ref_text.strip():
        if audio_hash in _ref_text_cache:
            show_info("Using cached reference text...")
            ref_text = _ref_text_cache[audio_hash]
        else:
            raise NotImplementedError("empty ref_text: the reference transcribes the clip with a Whisper ASR pipeline, which is not on this path")
    return path, normalize_ref_text(ref_text)


def remove_silence_pcm(pcm_int16, rate: int = 24000) -> np.ndarray:
    """`remove_silence_for_generated_wav` (F/infer/utils_infer.py:530-539) on mono int16 samples: `split_on_silence(min_silence_len=1000,
    silence_thresh=-50, keep_silence=500, seek_step=10)` and the pieces concatenated, so every pause of 1 s or more shrinks to the 500 ms
    on each side of it.  Like pydub's millisecond slicing, the result ends at `min(int(len_ms * rate / 1000), n)`: up to half a millisecond
    of samples past the last whole millisecond is dropped, and a wave without any pause comes back as that prefix.

    It acts on the int16 samples the routes emit, `rint(float32_wave * 32768)` clipped (`serve.pcm16`).  The reference runs the step on
    the file `sf.write` produced, and libsndfile's float -> PCM_16 scale may differ from that rule by one LSB; parity with it is unpinned,
    like the rest of this module."""
    pcm = np.asarray(pcm_int16)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise ValueError(f"remove_silence_pcm: mono int16 samples expected (got {pcm.dtype}, {pcm.ndim} dimensions)")
    pieces = split_on_silence(PcmSegment(pcm, rate), min_silence_len=1000, silence_thresh=-50, keep_silence=500, seek_step=10)
    if not pieces:
        return np.zeros(0, dtype=np.int16)
    return np.ascontiguousarray(np.concatenate([p.frames[:, 0] for p in pieces]))


# ------------------------------------------------------------------------------------------------ denoising an uploaded reference clip
# The definition of the per-voice `denoise` option (`infer.PreparedVoice(..., denoise=True)`; on the device `ops.ref_denoise`,
# csrc/ref_denoise.h): quantile-based noise estimation (Stahl, Fischer, Bippus 2000) with power spectral subtraction, on the front-end's
# output -- mono, 24 kHz, after the rms gain -- in float64:
#   window     w[i] = sin(pi i / 1024), the square root of the periodic Hann window, for analysis and synthesis; four shifts of w^2 by 256
#              sum to exactly 2
#   frames     F = ceil((n + 768) / 256); frame m holds clip samples 256 m - 768 .. 256 m + 255, zeros outside the clip: every clip sample
#              lies in exactly four frames
#   spectrum   X[m, k] = rfft(frame_m * w), k = 0 .. 512; P = re^2 + im^2
#   floor      r = (F - 1) // 5; floor[k] = the r-th smallest (0-based) of P[0 .. F - 1, k], no interpolation
#   smoothing  S[m, k] = the sum of P over frames m - 1 .. m + 1 and bins k - 1 .. k + 1, indices clamped to the edges (always nine terms), / 9
#   gain       G = max(0.125, (S - 6.75 floor[k]) / S) where S > 0, else 0.125
#   synthesis  y_m = irfft(G * X)[0 .. 1023] * w; out = overlap_add(y) / 2, cropped to the clip's n samples
# Every step is a continuous map of the samples, so the device's fp32 can be held to a tolerance.  6.75 is 1.5 times the bias
# -1 / ln(0.8) = 4.48 of the 20 % quantile of an exponentially distributed power, rounded to a dyadic value; the gain floor of 1/8 caps the
# attenuation at 18.06 dB.  The method treats whatever is there in every frame as noise: a buzz without pauses and with shallow modulation
# is damaged, which is why the option is per voice and off unless asked for.
DENOISE_N_FFT = 1024
DENOISE_HOP = 256
DENOISE_PAD = 768
DENOISE_RANK_DIV = 5
DENOISE_SUBTRACT = 6.75
DENOISE_MIN_GAIN = 0.125
DENOISE_MAX_SAMPLES = 1_440_000   # 60 s at 24 kHz


def check_denoise_length(n: int) -> None:
    """Refuses (ValueError) a clip of `n` samples at 24 kHz that the denoiser does not take."""
    if n > DENOISE_MAX_SAMPLES:
        raise ValueError(f"denoise: the reference clip has {n} samples at 24 kHz; at most DENOISE_MAX_SAMPLES = {DENOISE_MAX_SAMPLES} (60 s) are denoised")


def denoise_frames(n: int) -> int:
    return -(-(n + DENOISE_PAD) // DENOISE_HOP)


def denoise_floor(P: np.ndarray) -> np.ndarray:
    """floor[k]: the ((F - 1) // 5)-th smallest of P[:, k] (P [F, bins])."""
    r = (P.shape[0] - 1) // DENOISE_RANK_DIV
    return np.partition(P, r, axis=0)[r]


def denoise_reference(wave) -> np.ndarray:
    """The definition above of a mono 24 kHz clip `wave` [n] (or [1, n]), 1 <= n <= DENOISE_MAX_SAMPLES -> float32 [n]: `denoise_reference_f64`
    rounded once to the samples' format.  The length is preserved; a silent clip stays silent; and where floor[k] = 0 for every bin (a clean
    clip with pauses: G = 1 everywhere) the clip comes back up to rounding (a few 1e-16 relative in the float64 arithmetic), because
    sum_m w^2 = 2 over a sample's four frames."""
    return denoise_reference_f64(wave).astype(np.float32)


def denoise_reference_f64(wave) -> np.ndarray:
    """`denoise_reference` before its one rounding to float32: the definition's float64 samples [n]."""
    x = np.asarray(wave, dtype=np.float64).reshape(-1)
    n = len(x)
    if n < 1:
        raise ValueError("denoise: the reference clip is empty")
    check_denoise_length(n)
    N, H = DENOISE_N_FFT, DENOISE_HOP
    F = denoise_frames(n)
    w = np.sin(np.pi * np.arange(N) / N)
    xp = np.zeros(H * (F - 1) + N)
    xp[DENOISE_PAD:DENOISE_PAD + n] = x
    X = np.fft.rfft(np.lib.stride_tricks.sliding_window_view(xp, N)[::H] * w, axis=1)
    P = X.real ** 2 + X.imag ** 2
    floor = denoise_floor(P)
    Pe = np.pad(P, 1, mode="edge")
    S = np.zeros_like(P)
    for dm in range(3):
        for dk in range(3):
            S += Pe[dm:dm + F, dk:dk + P.shape[1]]
    S /= 9.0
    G = np.full_like(S, DENOISE_MIN_GAIN)
    np.divide(S - DENOISE_SUBTRACT * floor, S, out=G, where=S > 0)
    G = np.maximum(G, DENOISE_MIN_GAIN)
    y = np.fft.irfft(G * X, n=N, axis=1) * w
    out = np.zeros_like(xp)
    for m in range(F):
        out[H * m:H * m + N] += y[m]
    return out[DENOISE_PAD:DENOISE_PAD + n] / 2.0


# ------------------------------------------------------------------------------------------------ is an uploaded reference clip fit to clone from?
# The definition of the reference-clip report (`infer.PreparedVoice(..., assess=True)`, `TTSManager.check_reference`, the upload gate
# `TTSManager(reference_limits=...)`; on the device `ops.ref_assess`, csrc/ref_assess.h).  `raw` is the clip the front-end is handed,
# float32 [ch, n] at its own rate; `prepared` is the front-end's output, mono at 24 kHz.
#   peak         max |x| over all channels of raw, a float32 value
#   hot          |x| >= peak * (1 - 2^-10), one float32 product and comparison (16-bit PCM tops at 32767 / 32768 against -1.0: both are hot)
#   clipped      the hot samples that lie in a run of at least 3 consecutive hot samples WITHIN ONE CHANNEL: sample j counts when it is hot and
#                (j - 1 and j + 1) or (j - 1 and j - 2) or (j + 1 and j + 2) are, a position outside the channel never being hot.  0 when
#                peak < 0.25 (a quiet recording's tops are its loudest syllables, not the converter's rails) and 0 when EVERY sample is hot
#                (zeros, DC, a full-scale square wave: there is no waveform to have been clipped)
#   clip_ratio   clipped / (ch n), float64
#   spectrum     the first ASSESS_MAX_SAMPLES samples of prepared, framed exactly as the denoiser frames them (sqrt-Hann frames of 1024 at
#                hop 256 behind 768 zeros): P[f][k], F frames, floor[k] = the ((F - 1) // 5)-th smallest of P[.][k]
#   band B       bins 3 .. 341 (70 Hz .. 8 kHz); E[f] = sum_{k in B} P[f][k], ascending k
#   N            ASSESS_FLOOR_TO_MEAN * sum_{k in B} floor[k] (ascending k), ASSESS_FLOOR_TO_MEAN = -1 / ln(0.8) = 4.4814: the 20 % quantile of
#                an exponentially distributed power is 0.2231 of its mean, so N estimates the mean noise power of a frame in the band
#   S            (1 / F) * sum_f E[f], ascending f: the mean power of a frame in the band, noise included
#   noise_db     10 log10(N); -inf when N == 0
#   snr_db       10 log10(max(S - N, 0) / N); +inf when N == 0, -inf when S <= N
#   speech_ratio the share of frames with E[f] >= 4 N and E[f] > 0
#   bandwidth_hz m[k] = the mean over frames of the mean of P[f][k .. k + 7], k = 0 .. 505; k* = the largest k with m[k] >= 1e-5 max m;
#                (k* + 8) * 24000 / 1024: the upper edge of the highest 8-bin window that still holds a 100 000th of the strongest one's
#                power.  0 for an all-zero clip
#   seconds, rms the front-end's values, handed through
# The weak case is the denoiser's: a voice WITHOUT PAUSES has its own speech as the floor, so N is too high, `snr_db` reads low and
# `speech_ratio` reads the share of frames above four times the speech's own quantile, which says nothing.  S includes the pauses, so a clip
# that is 40 % pause reads 2.2 dB below the SNR of its speech alone.  Calibration on synthetic hosts: DESIGN.md §8.  No built-in thresholds:
# `reference_limits` are the operator's.
ASSESS_MAX_SAMPLES = DENOISE_MAX_SAMPLES
ASSESS_HOT = 1.0 - 2.0 ** -10
ASSESS_MIN_PEAK = 0.25
ASSESS_MIN_RUN = 3
ASSESS_BAND = (3, 341)
ASSESS_FLOOR_TO_MEAN = -1.0 / math.log(0.8)
ASSESS_SPEECH_FACTOR = 4.0
ASSESS_MEAN_BINS = 8
ASSESS_BANDWIDTH_REL = 1e-5
ASSESS_MAX_CHANNELS = 8
ASSESS_ROW = ("clipped", "peak_bits", "speech_frames", "k_star", "N", "S", "noise_db", "snr_db", "speech_ratio", "bandwidth_hz")
REFERENCE_LIMITS = ("min_seconds", "max_clip_ratio", "min_snr_db", "min_speech_ratio", "min_bandwidth_hz")


class ReferenceReport(typing.NamedTuple):
    """The measures of one reference clip (the definition above).  `rms` is None where no front-end value was handed in."""
    seconds: float
    rms: float | None
    peak: float
    clipped: int
    clip_ratio: float
    noise_db: float
    snr_db: float
    speech_ratio: float
    bandwidth_hz: float

    def as_json(self) -> dict:
        """The report as a JSON object: an infinite `noise_db` / `snr_db` is null."""
        return {k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in self._asdict().items()}


def check_reference_limits(limits):
    """`TTSManager(reference_limits=...)` checked: None, or a dict of `REFERENCE_LIMITS` names to finite numbers -> a dict of floats.
    ValueError for an unknown name or a value that is not a number."""
    if limits is None:
        return None
    if not isinstance(limits, dict):
        raise ValueError(f"reference_limits must be a dict of {', '.join(REFERENCE_LIMITS)} (got {type(limits).__name__})")
    out = {}
    for name, value in limits.items():
        if name not in REFERENCE_LIMITS:
            raise ValueError(f"reference_limits: unknown limit {name!r} (known: {', '.join(REFERENCE_LIMITS)})")
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
            raise ValueError(f"reference_limits: {name} must be a finite number (got {value!r})")
        out[name] = float(value)
    return out


def reference_problems(report: ReferenceReport, limits, denoise: bool = False) -> list:
    """The limits of `limits` (a checked dict, or None) that `report` violates, one sentence each, naming the measure, its value and the
    limit.  `min_snr_db` is not applied to a voice with `denoise`: the denoiser is the remedy."""
    problems = []
    for name, limit in (limits or {}).items():
        kind, measure = name.split("_", 1)
        if measure == "snr_db" and denoise:
            continue
        value = getattr(report, measure)
        if (value < limit) if kind == "min" else (value > limit):
            problems.append(f"the reference clip's {measure} is {value:.6g}, {'below' if kind == 'min' else 'above'} the limit {name} = {limit:.6g}")
    return problems


def assess_clipping(raw):
    """(peak float32, clipped int) of raw [ch, n] by the definition above."""
    x = np.abs(np.asarray(raw, dtype=np.float32))
    x = x.reshape(1, -1) if x.ndim == 1 else x
    if x.ndim != 2 or x.shape[1] < 1 or not 1 <= x.shape[0] <= ASSESS_MAX_CHANNELS:
        raise ValueError(f"assess: the clip must be [1 .. {ASSESS_MAX_CHANNELS} channels, at least one sample] (got {x.shape})")
    peak = np.float32(x.max())
    hot = x >= peak * np.float32(ASSESS_HOT)
    if peak < np.float32(ASSESS_MIN_PEAK) or hot.all():
        return peak, 0
    h = np.pad(hot, ((0, 0), (2, 2)))                     # outside the channel: never hot
    l2, l1, me, r1, r2 = (h[:, i:i + x.shape[1]] for i in range(5))
    return peak, int(np.count_nonzero(me & ((l1 & r1) | (l1 & l2) | (r1 & r2))))


def denoise_power(x: np.ndarray) -> np.ndarray:
    """P [F, 513] of a mono clip x [n] float64: the power of the denoiser's frames (`denoise_reference_f64`'s framing and window)."""
    N, H = DENOISE_N_FFT, DENOISE_HOP
    F = denoise_frames(len(x))
    w = np.sin(np.pi * np.arange(N) / N)
    xp = np.zeros(H * (F - 1) + N)
    xp[DENOISE_PAD:DENOISE_PAD + len(x)] = x
    X = np.fft.rfft(np.lib.stride_tricks.sliding_window_view(xp, N)[::H] * w, axis=1)
    return X.real ** 2 + X.imag ** 2


def assess_spectrum(prepared) -> dict:
    """The spectral measures of a prepared 24 kHz mono wave by the definition above, with the intermediate values the tests read:
    dict(F, E, N, S, noise_db, snr_db, speech_frames, speech_ratio, m, k_star, bandwidth_hz)."""
    x = np.asarray(prepared, dtype=np.float64).reshape(-1)[:ASSESS_MAX_SAMPLES]
    if len(x) < 1:
        raise ValueError("assess: the reference clip is empty")
    P = denoise_power(x)
    F, (b0, b1) = P.shape[0], ASSESS_BAND
    E = np.cumsum(P[:, b0:b1 + 1], axis=1)[:, -1]                              # ascending k
    N = ASSESS_FLOOR_TO_MEAN * float(np.cumsum(denoise_floor(P)[b0:b1 + 1])[-1])
    S = float(np.cumsum(E)[-1]) / F                                            # ascending f
    speech = int(np.count_nonzero((E >= ASSESS_SPEECH_FACTOR * N) & (E > 0)))
    m = np.lib.stride_tricks.sliding_window_view(P, ASSESS_MEAN_BINS, axis=1).mean(axis=2).mean(axis=0)
    top = float(m.max())
    k_star = int(np.flatnonzero(m >= ASSESS_BANDWIDTH_REL * top)[-1]) if top > 0 else -1
    return dict(F=F, E=E, m=m, speech_frames=speech, k_star=k_star, **assess_ratios(N, S, speech, F, k_star))


def assess_ratios(N: float, S: float, speech_frames: int, F: int, k_star: int) -> dict:
    """N, S, the count of speech frames and k* -> dict(N, S, noise_db, snr_db, speech_ratio, bandwidth_hz)."""
    noise_db = 10.0 * math.log10(N) if N > 0 else -math.inf
    snr_db = math.inf if not N > 0 else (10.0 * math.log10((S - N) / N) if S > N else -math.inf)
    return dict(N=N, S=S, noise_db=noise_db, snr_db=snr_db, speech_ratio=speech_frames / F,
                bandwidth_hz=(k_star + ASSESS_MEAN_BINS) * 24000.0 / DENOISE_N_FFT if k_star >= 0 else 0.0)


def assess_reference(raw, sr, prepared, rms=None) -> ReferenceReport:
    """The report of one clip by the definition above: `raw` float32 [ch, n] at `sr` Hz as the front-end is handed it, `prepared` the
    front-end's 24 kHz mono wave [nw] (or [1, nw]); `rms`: the front-end's measured rms, handed through (None: not reported).  Degenerate
    clips have defined values: zeros (clipped 0, N = S = 0, noise_db -inf, snr_db +inf, speech_ratio 0, bandwidth 0), DC (clipped 0), one
    sample (F = 4 frames, rank 0: the floor is each bin's smallest power)."""
    raw = np.asarray(raw, dtype=np.float32)
    raw = raw.reshape(1, -1) if raw.ndim == 1 else raw
    peak, clipped = assess_clipping(raw)
    s = assess_spectrum(prepared)
    return ReferenceReport(seconds=raw.shape[1] / sr, rms=None if rms is None else float(rms), peak=float(peak), clipped=clipped,
                           clip_ratio=clipped / float(raw.size), noise_db=s["noise_db"], snr_db=s["snr_db"], speech_ratio=s["speech_ratio"],
                           bandwidth_hz=s["bandwidth_hz"])


def report_from_row(row, seconds, rms, samples) -> ReferenceReport:
    """One row of `ops.ref_assess` (int64 [len(ASSESS_ROW)], the float64 values as their bit patterns) -> the report; `samples` = ch * n of raw."""
    row = np.ascontiguousarray(row, dtype=np.int64)
    f = dict(zip(ASSESS_ROW, row.view(np.float64).tolist()))
    clipped = int(row[0])
    return ReferenceReport(seconds=float(seconds), rms=None if rms is None else float(rms),
                           peak=float(np.array([row[1]], dtype=np.int64).astype(np.uint32).view(np.float32)[0]), clipped=clipped,
                           clip_ratio=clipped / float(samples), noise_db=f["noise_db"], snr_db=f["snr_db"], speech_ratio=f["speech_ratio"],
                           bandwidth_hz=f["bandwidth_hz"])
