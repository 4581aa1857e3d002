"""Drop-in mirror of the reference's inference driver (F/infer/utils_infer.py): module constants (:40-53),
`chunk_text` (:61-88), `infer_process` (:357-400) and `infer_batch_process` (:406-524), with the same
signatures, defaults, return triple and quirks (UTF-8 byte budgets, `ref_audio_len = nw // 256`, float64
cross-fade ramps), running the sampler and vocoder on the HIP objects (`F5HipModel`, `F5HipVocos`).  Also the
reference's speech-edit script (F/infer/speech_edit.py:119-192) as `plan_edit` / `speech_edit` / `speech_edit_batch`.

Host-side differences, all explicit:
  * reference audio is read by `wave_codec.load_audio`: WAV through `load_wav` (a RIFF chunk walker: PCM 8/16/24/32-bit, IEEE float
    32/64-bit, WAVE_FORMAT_EXTENSIBLE), native FLAC through `read_flac` (the whole format in Python integers; `ops.flac_decode` is the
    same function on the device), or passed as a `(tensor, sr)` pair: torchaudio is not part of this image;
  * resampling to 24 kHz restates torchaudio.transforms.Resample (sinc interpolation, Hann window, width 6, rolloff 0.99; third-party
    leaf, parity unpinned) on the host, like the reference does before `.to(device)`: `wave_codec.resample_sinc_hann`;
  * what the driver has no counterpart for -- WAV reading, the resamplers and their tap tables, G.711, the delivery format of a request --
    lives in the leaf module `wave_codec`; its public names are handed on here (`infer.load_wav`, `infer.deliver_pcm16`, ...);
  * `preprocess_ref_audio_text` (silence clipping of the reference clip, ". " rule) is restated without pydub in `audio_prep.py`;
  * `convert_char_to_pinyin` (jieba + pypinyin) is replaced by `text_to_tokens`, which reproduces the reference's
    behaviour for text without CJK characters (per-character tokens, the same punctuation translation table)
    and rejects CJK input instead of silently mis-tokenising it.
"""
from __future__ import annotations

import collections
import contextlib
import dataclasses
import math
import re
import types
from dataclasses import dataclass

import numpy as np
import torch

from . import wave_codec
from .audio_prep import preprocess_ref_audio_text, remove_silence_edges, remove_silence_pcm  # noqa: F401  (F/infer/utils_infer.py:263-350)
from .audio_prep import DENOISE_MAX_SAMPLES, check_denoise_length, denoise_reference  # noqa: F401  (the per-voice `denoise` option of an uploaded clip)
from .audio_prep import (ASSESS_MAX_SAMPLES, REFERENCE_LIMITS, ReferenceReport, assess_reference, check_reference_limits,  # noqa: F401
                         reference_problems, report_from_row)   # (the reference-clip report and the upload gate)
from .loaders import DiT, MMDiT, UNetT, load_checkpoint, load_model, load_vocoder  # noqa: F401  (F/infer/utils_infer.py:92-130,175-260)
from .wave_codec import (ALL_ENCODINGS, DELIVERY_OPTIONS, FLAC_BLOCK, FLAC_ENCODINGS, FLAC_HEADER_BYTES, MAX_TAP_TABLE_BYTES, OUTPUT_ENCODINGS,  # noqa: F401
                         OUTPUT_SAMPLE_RATES, TAP_TABLE_CACHE, WAVE_OPTIONS, WHOLE_WAVE, WHOLE_WAVE_LOUDNESS, StreamDelivery, StreamFlacEncoder,
                         StreamResampler, WaveSpec, check_flac_level, decode_flac, decode_g711, deliver_pcm16,
                         delivery_format, encode_flac, encode_g711, flac_crc8, flac_crc16, flac_stream_header, load_audio, load_wav, quantise_pcm16, read_flac,
                         rate_pair, request_flac_level, resample_pcm16, resample_sinc_hann, resample_taps, resampled_length)   # (handed on: every public name of wave_codec is infer.X too)
from .wave_codec import FORMANT_OPTIONS, check_keep_formants, formant_stretch, psola_pcm16  # noqa: F401
from .wave_codec import (PITCH_RANGE, PITCH_RATIOS, PROSODY_OPTIONS, WHOLE_WAVE_PROSODY, check_pitch, check_tempo, shift_pcm16,  # noqa: F401
                         shifted_length, wsola_pcm16)
from .wave_codec import (WATERMARK_BAND, WATERMARK_BLOCK, WATERMARK_KEYS_MAX, WATERMARK_MAX_SAMPLES, WATERMARK_MIN_SAMPLES,  # noqa: F401
                         WATERMARK_OPTIONS, WATERMARK_PERIOD, WATERMARK_SHIFT, WATERMARK_TAPS, WATERMARK_THRESHOLD, WHOLE_WAVE_WATERMARK,
                         WatermarkScore, check_watermark, check_watermark_keys, detect_watermark, mark_pcm16, watermark_carrier)
from .wave_codec import (WATERMARK_ID_BITS, WATERMARK_ID_KEYS_MAX, WATERMARK_ID_MAX, WATERMARK_ID_THRESHOLD, WatermarkRead, WatermarkTag,  # noqa: F401
                         check_watermark_id, read_watermark, watermark_key, watermark_subkey)
from .wave_codec import (WATERMARK_SCAN_MAX_SAMPLES, WATERMARK_SCAN_SLACK, WATERMARK_SCAN_WINDOW, WatermarkRange, WatermarkSpan,  # noqa: F401
                         scan_watermark, watermark_spans, watermark_windows)
from .wave_codec import (LOUDNESS_GATE_ABS, LOUDNESS_PEAK_CEILING, LOUDNESS_RANGE, LOUDNESS_TAPS, check_loudness, loudness_gain,  # noqa: F401
                         loudness_gain_constant, loudness_lufs, loudness_taps, measure_loudness, normalise_loudness_pcm16)
from .wave_codec import _device_taps, _tap_tables  # noqa: F401  (the two caches: used below, and read as infer._X by the tests that bound them)

# ----------------------------------------- F/infer/utils_infer.py:40-53
target_sample_rate = 24000
n_mel_channels = 100
hop_length = 256
win_length = 1024
n_fft = 1024
mel_spec_type = "vocos"
target_rms = 0.1
cross_fade_duration = 0.15
ode_method = "euler"
nfe_step = 32
cfg_strength = 2.0
sway_sampling_coef = -1.0
speed = 1.0
fix_duration = None
span_steps = 8   # SpanScheduler: ODE steps per span (profiles/r07_admission_bench.txt; DESIGN.md "Resumable spans")
assert target_sample_rate == wave_codec.SAMPLE_RATE   # wave_codec is a leaf module and keeps its own constant


def chunk_text(text, max_chars=135):
    """F/infer/utils_infer.py:61-88: split at punctuation, greedily pack sentences by UTF-8 byte budget."""
    chunks = []
    current = ""
    for sentence in re.split(r"(?<=[;:,.!?])\s+|(?<=[；：，。！？])", text):
        piece = sentence + " " if sentence and len(sentence[-1].encode("utf-8")) == 1 else sentence
        if len(current.encode("utf-8")) + len(sentence.encode("utf-8")) <= max_chars:
            current += piece
        else:
            if current:
                chunks.append(current.strip())
            current = piece
    if current:
        chunks.append(current.strip())
    return chunks


_CUSTOM_TRANS = str.maketrans({";": ",", "“": '"', "”": '"', "‘": "'", "’": "'"})   # F/model/utils.py:142-144

# jieba 0.42.1 `cut(text)` (default mode, HMM on) restated for text WITHOUT CJK characters (third-party leaf, absent here: parity
# unpinned, known-answer tests in tests/test_host_glue.py).  Its published algorithm: blocks matching re_han_default go to the
# dictionary cutter, everything else is split at whitespace and yielded character by character; inside a block every character that
# starts no dictionary word is buffered and the buffer goes through finalseg.cut, whose non-Han path splits at re_skip -- runs of
# [a-zA-Z0-9]+(.digits)?%? stay whole and so do the runs of "+#&._%-" between them.  (jieba's dictionary holds a handful of entries
# with Latin letters, e.g. "AT&T", "C++": those would come out as one segment there and as several here.)
_RE_HAN_DEFAULT = re.compile(r"([\u4E00-\u9FD5a-zA-Z0-9+#&\._%\-]+)")
_RE_SKIP_DEFAULT = re.compile(r"(\r\n|\s)")
_RE_SKIP_FINAL = re.compile(r"([a-zA-Z0-9]+(?:\.\d+)?%?)")


def _segments_non_cjk(text):
    for blk in _RE_HAN_DEFAULT.split(text):
        if not blk:
            continue
        if _RE_HAN_DEFAULT.match(blk):
            if len(blk) == 1:
                yield blk
            else:
                yield from (x for x in _RE_SKIP_FINAL.split(blk) if x)
        else:
            for x in _RE_SKIP_DEFAULT.split(blk):
                if _RE_SKIP_DEFAULT.match(x):
                    yield x
                else:
                    yield from x


def text_to_tokens(text_list):
    """convert_char_to_pinyin (F/model/utils.py:140-177) for text without CJK characters: translation table, jieba-style
    segmentation, then the reference's rule per segment -- a pure-ASCII segment longer than one character gets a space in front
    unless the previous token is one of space, colon, quote (:153-156), and is spelled out character by character; every other
    segment (Indic scripts arrive one character per segment, and pypinyin returns non-Han characters unchanged) passes through
    character by character.  CJK input is rejected instead of silently mis-tokenised (the pinyin front-end needs jieba's dictionary
    and pypinyin's tables, which are not available offline)."""
    out = []
    for text in text_list:
        text = text.translate(_CUSTOM_TRANS)
        if any("\u3100" <= c <= "\u9fff" for c in text):
            raise NotImplementedError("CJK text needs the pinyin front-end (jieba/pypinyin), which is not on this path yet")
        chars = []
        for seg in _segments_non_cjk(text):
            if len(seg.encode("utf-8")) == len(seg) and chars and len(seg) > 1 and chars[-1] not in " :'\"":
                chars.append(" ")
            chars.extend(seg)
        out.append(chars)
    return out


def infer_process(ref_audio, ref_text, gen_text, model_obj, vocoder, mel_spec_type=mel_spec_type, show_info=print,
                  progress=None, target_rms=target_rms, cross_fade_duration=cross_fade_duration, nfe_step=nfe_step,
                  cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, speed=speed,
                  fix_duration=fix_duration, device=None, seed=None, ode_method=None):
    """F/infer/utils_infer.py:357-400.  `seed` (not in the reference's signature): the request's noise comes from its own CPU generator
    (`request_generator`) instead of the global one.  `ode_method` (neither): "euler", "midpoint" or "rk4" for this request instead of the
    model object's solver."""
    audio, sr = ref_audio if isinstance(ref_audio, tuple) else load_audio(ref_audio)
    gen_text_batches = request_chunks(ref_text, audio.shape[-1] / sr, gen_text)
    return infer_batch_process((audio, sr), ref_text, gen_text_batches, model_obj, vocoder, mel_spec_type=mel_spec_type,
                               progress=progress, target_rms=target_rms, cross_fade_duration=cross_fade_duration,
                               nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef,
                               speed=speed, fix_duration=fix_duration, device=device, seed=seed, ode_method=ode_method)


def request_chunks(ref_text, ref_seconds, gen_text):
    """The text chunks of one request (F/infer/utils_infer.py:379-381): a UTF-8 byte budget proportional to the reference's
    bytes per second over what is left of 25 s, then `chunk_text`.  `ref_seconds` is the reference clip's length before resampling."""
    max_chars = int(len(ref_text.encode("utf-8")) / ref_seconds * (25 - ref_seconds))
    return chunk_text(gen_text, max_chars=max_chars)


def infer_process_stream(ref_audio, ref_text, gen_text, model_obj, vocoder, mel_spec_type=mel_spec_type, show_info=print,
                         progress=None, target_rms=target_rms, cross_fade_duration=cross_fade_duration, nfe_step=nfe_step,
                         cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, speed=speed,
                         fix_duration=fix_duration, device=None, seed=None, ode_method=None):
    """`infer_process` as a generator of float32 pieces at 24 kHz whose concatenation is `infer_process`'s wave (as float32).

    The text is chunked exactly as `infer_process` does; chunk 0 is sampled and vocoded alone and its stable samples are yielded, then
    the remaining chunks are sampled in ONE `sample_units` call and the rest follows (`StreamJoiner`: the last fade length of what has
    been joined is held back until the next chunk's cross-fade is known).  Every chunk is an independent unit with batch-1 semantics and
    noise is drawn unit by unit in order, so with the model handle in shape-invariant attention mode and the same generator state before
    both calls (`torch.manual_seed`), the pieces equal `infer_process`'s wave to the last bit.  With `seed`, both calls draw from the
    request's one generator (the remaining chunks after the first chunk's draws), so the pieces equal `infer_process(..., seed=seed)`."""
    audio, sr = ref_audio if isinstance(ref_audio, tuple) else load_audio(ref_audio)
    voice, units = _plan_request((audio, sr), ref_text, gen_text, target_rms, speed, fix_duration, device, text_to_tokens)
    knobs = dict(steps=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, ode_method=ode_method)
    gen = request_generator(seed)
    joiner = StreamJoiner(cross_fade_duration)
    for part in (units[:1], units[1:]):
        if not part:
            continue
        mels = _sample(model_obj, voice, part, knobs, gen)
        (waves, _), = _chunk_waves([(mels, voice.ref_frames, voice.rms)], vocoder, mel_spec_type, target_rms)
        yield from joiner.pieces(waves)
    yield from joiner.pieces(flush=True)


def _prepare_reference(audio, sr, rms_floor, device):
    """Prologue of infer_batch_process (F/infer/utils_infer.py:423-433): mono mix, gain up to `rms_floor`, resample to 24 kHz.
    Returns (audio [1, nw] fp32, measured rms)."""
    if audio.shape[0] > 1:
        audio = torch.mean(audio, dim=0, keepdim=True)
    rms = torch.sqrt(torch.mean(torch.square(audio)))
    if rms < rms_floor:
        audio = audio * rms_floor / rms
    if sr != target_sample_rate:
        audio = resample_sinc_hann(audio, sr, target_sample_rate)
    if device is not None:
        audio = audio.to(device)
    return audio, rms


def plan_units(ref_text, gen_text_batches, ref_frames, speed=1.0, fix_duration=None, tokenizer=None):
    """One sampling unit per text chunk: (tokens of ref_text + chunk, total frames).  Duration rule of the reference
    (F/infer/utils_infer.py:446-454): UTF-8 byte lengths, `ref_frames = n_samples // hop` (one less than the mel has: SURVEY B2)."""
    tokenizer = tokenizer or text_to_tokens
    ref_bytes = len(ref_text.encode("utf-8"))
    units = []
    for chunk in gen_text_batches:
        if fix_duration is not None:
            frames = int(fix_duration * target_sample_rate / hop_length)
        else:
            frames = ref_frames + int(ref_frames / ref_bytes * len(chunk.encode("utf-8")) / speed)
        units.append((tokenizer([ref_text + chunk])[0], frames))
    return units


def cross_fade_concat(waves, fade_seconds, sample_rate=target_sample_rate):
    """Joins the chunk waveforms (F/infer/utils_infer.py:485-519): plain concatenation for a non-positive fade, else a linear
    cross-fade over min(fade, len(prev), len(next)) samples.  The ramps are float64 (np.linspace), so the result is float64 from the
    second chunk on, exactly like the reference's."""
    if fade_seconds <= 0:
        return np.concatenate(waves)
    out = waves[0]
    for nxt in waves[1:]:
        out = _cross_fade(out, nxt, int(fade_seconds * sample_rate))
    return out


def _cross_fade(out, nxt, fade):
    """One join of `cross_fade_concat`: `nxt` behind `out`, faded over n = min(fade, len(out), len(nxt)) samples (n <= 0: appended)."""
    n = min(fade, len(out), len(nxt))
    if n <= 0:
        return np.concatenate([out, nxt])
    ramp = np.linspace(0, 1, n)
    return np.concatenate([out[:-n], out[-n:] * ramp[::-1] + nxt[:n] * ramp, nxt[n:]])


class StreamJoiner:
    """`cross_fade_concat` one chunk wave at a time.  A later cross-fade rewrites at most the last int(fade_seconds * sample_rate)
    samples of what has been joined so far (n = min(fade, len(out), len(next))), so `push(wave)` returns the samples that can no longer
    change and holds back that many; `flush()` returns the rest.  The concatenation of every returned piece is `np.array_equal` to
    `cross_fade_concat(waves, fade_seconds)`, dtype included (float64 from the first cross-fade on, like the reference's)."""

    def __init__(self, fade_seconds, sample_rate=target_sample_rate):
        self.fade = int(fade_seconds * sample_rate) if fade_seconds > 0 else 0
        self.total = 0          # samples of the joined wave so far, emitted and held
        self.held = None        # its last min(fade, total) samples

    def push(self, wave):
        nxt = np.asarray(wave)
        if self.held is None:
            local = nxt
        else:
            local = _cross_fade(self.held, nxt, self.fade)
            self.total -= len(self.held)
        self.total += len(local)
        keep = min(self.fade, self.total)          # <= len(local): see the class note
        self.held = local[len(local) - keep:]
        return local[:len(local) - keep]

    def flush(self):
        held, self.held = self.held, None
        return held if held is not None else np.zeros(0, dtype=np.float32)

    def cut(self):
        """A butt join (`join_segments`: between two pieces of a script, around a gap): releases what is held -- nothing fades into it any
        more -- and the next `push` starts without a fade, like the first one."""
        self.total = 0
        return self.flush()

    def pieces(self, waves=(), flush=False, cut=False):
        """What a stream hands on: the non-empty pieces that pushing `waves` one after the other releases -- with `flush` or `cut`, the held
        rest behind them -- each as float32."""
        for wave in waves:
            piece = self.push(wave)
            if len(piece):
                yield np.asarray(piece, dtype=np.float32)
        if flush or cut:
            piece = self.cut() if cut else self.flush()
            if len(piece):
                yield np.asarray(piece, dtype=np.float32)


def join_segments(chunk_waves_per_segment, cross_fade_duration=cross_fade_duration, gap_samples=0):
    """The wave of a multi-voice script (F/infer/infer_cli.py:198-208): `np.concatenate` of `cross_fade_concat(segment)` per segment -- the
    chunks of one voice's piece are cross-faded, the pieces butt against each other -- with `gap_samples` float32 zeros between consecutive
    segments (0: the reference's `np.concatenate` exactly), as float32 like `request_wave`."""
    parts = []
    for i, waves in enumerate(chunk_waves_per_segment):
        if i and gap_samples > 0:
            parts.append(np.zeros(int(gap_samples), dtype=np.float32))
        parts.append(cross_fade_concat(list(waves), cross_fade_duration))
    return np.asarray(np.concatenate(parts), dtype=np.float32)


MAX_SCRIPT_SEGMENTS = 64
MAX_SCRIPT_GAP = 5.0   # seconds


def check_script_gap(gap) -> float:
    """A script's `gap` in seconds, refused with ValueError unless it is a number with 0 <= gap <= `MAX_SCRIPT_GAP`."""
    if isinstance(gap, bool) or not isinstance(gap, (int, float)) or not (math.isfinite(gap) and 0 <= gap <= MAX_SCRIPT_GAP):
        raise ValueError(f"gap must be a number of seconds between 0 and {MAX_SCRIPT_GAP:g} (got {gap!r})")
    return float(gap)


class ScriptRequest:
    """A multi-voice script as ONE request, accepted wherever `infer_requests`, `SpanScheduler.admit` and `SpanScheduler.prepare` accept a
    request tuple: `segments` = [(ref_audio | PreparedVoice, ref_text, text[, speed])], one per piece in order, each planned like a plain
    request with its own voice, chunking and (optionally) speed; `options` as a plain request's fourth element (`REQUEST_OPTIONS`: they
    hold for every segment, `speed` where a segment names none, and `remove_silence` / `sample_rate` / `encoding` apply to the joined
    script); `gap`: seconds of silence between consecutive segments, 0 <= gap <= 5, int(gap * 24000) samples.  Its result is
    `join_segments` of its segments' chunk waves, finished like a plain request's joined wave.  With every `text` a list of chunk texts
    (a streamed script's tail) the result is the per-chunk waves, one list per segment, for the caller's cut-aware `StreamJoiner`.
    Refused here with ValueError: no segment or more than 64, a malformed segment, an empty text, texts of both kinds, a gap out of range."""

    def __init__(self, segments, options=None, gap=0.0):
        segments = [tuple(seg) for seg in segments]
        if not 1 <= len(segments) <= MAX_SCRIPT_SEGMENTS:
            raise ValueError(f"a script needs between 1 and {MAX_SCRIPT_SEGMENTS} pieces (got {len(segments)})")
        for i, seg in enumerate(segments):
            if len(seg) not in (3, 4):
                raise ValueError(f"script segment {i}: expected (ref_audio, ref_text, text[, speed]), got {len(seg)} elements")
            text = seg[2]
            if isinstance(text, (list, tuple)):
                ok = len(text) > 0 and all(isinstance(t, str) and t.strip() for t in text)
            else:
                ok = isinstance(text, str) and bool(text.strip())
            if not ok:
                raise ValueError(f"script segment {i} has no text to synthesize")
            if not isinstance(seg[1], str) or not seg[1].strip():
                raise ValueError(f"script segment {i}: the reference text cannot be empty")
            if len(seg) == 4 and seg[3] is not None and not (isinstance(seg[3], (int, float)) and math.isfinite(seg[3]) and seg[3] > 0):
                raise ValueError(f"script segment {i}: speed must be a positive number (got {seg[3]!r})")
        kinds = {isinstance(seg[2], (list, tuple)) for seg in segments}
        if len(kinds) > 1:
            raise ValueError("a script's texts are all strings, or all lists of chunk texts (a streamed script's tail)")
        self.segments, self.options, self.gap = segments, dict(options or {}), check_script_gap(gap)
        self.chunked = kinds.pop()

    @property
    def gap_samples(self) -> int:
        return int(self.gap * target_sample_rate)

    @property
    def text(self):
        """What `finish_requests` takes as the request's text: a list (per-chunk waves come back) for a chunked script, else a string."""
        return [seg[2] for seg in self.segments] if self.chunked else " ".join(seg[2] for seg in self.segments)


class SegmentedWaves(list):
    """The chunk waves of a script request for `finish_requests`: one list of chunk waves per segment, and the gap between segments."""

    def __init__(self, segments, gap_samples=0):
        super().__init__(list(waves) for waves in segments)
        self.gap_samples = int(gap_samples)


def request_voices(request):
    """The reference voices of a request tuple or `ScriptRequest` as they were handed in (paths, pairs, `PreparedVoice`s), one per segment."""
    return [seg[0] for seg in request.segments] if isinstance(request, ScriptRequest) else [request[0]]


def request_text(request):
    return request.text if isinstance(request, ScriptRequest) else request[2]


def request_chunk_waves(plan, groups):
    """`_chunk_waves`' output for a plan's groups -> what `finish_requests` takes for the request."""
    waves = [w for w, _ in groups]
    return SegmentedWaves(waves, plan.script.gap_samples) if plan.script is not None else waves[0]


class PreparedVoice:
    """The per-voice part of `infer_process` done once: the reference wave after mono mix / rms gain / resampling
    (F/infer/utils_infer.py:423-433), its measured rms, its duration in seconds before resampling (the `max_chars` rule, :379) and --
    filled in by the first request that uses it -- the reference mel on the device (the "reference latents": 188 KB for a 5 s
    prompt).  `serve.TTSManager` keeps one per voice; `infer_requests` accepts it wherever a `ref_audio` is expected.

    `PreparedVoice.deferred((wave, sr), target_rms)` is the same voice before any arithmetic on its samples: `seconds` and `ref_frames`
    follow from the clip's length alone (so a request can be planned), `audio` / `rms` / `mel` are filled in by `prepare_voices` -- one
    ragged front-end call on the device for all deferred voices of a batch (`infer_requests`, `SpanScheduler`).

    `denoise` (False): the voice's wave goes through `audio_prep.denoise_reference` behind the front-end -- for recordings with hiss, fan
    noise or hum.  `rms`, `seconds` and `ref_frames` stay the front-end's; a clip longer than `DENOISE_MAX_SAMPLES` at 24 kHz is refused
    by both constructors.  A deferred voice is denoised by `prepare_voices`: on the device in one `ops.ref_denoise` call per front-end call.

    `reject_marked` (None): watermark keys the clip must not carry.  The prepared 24 kHz wave is scored against them before the denoiser
    (`check_unmarked`; a deferred voice by `prepare_voices`: on the device in one `ops.watermark_detect` call per front-end call), and a
    clip that scores at or above `WATERMARK_THRESHOLD` for any key is a ValueError (`MARKED_REFERENCE`).

    `assess` (False): the clip is measured (`audio_prep.assess_reference`: clipping, noise floor, SNR, speech share, bandwidth) on the clip
    the front-end is handed and its 24 kHz output, in front of the watermark check and the denoiser, and `report` holds the
    `ReferenceReport`; it stays None until measured (a deferred voice: by `prepare_voices`, on the device in one `ops.ref_assess` call per
    front-end call).  `limits` (None): a dict of `REFERENCE_LIMITS`; it implies `assess`, and a clip that violates one is a ValueError
    naming the measure, its value and the limit (`min_snr_db` is not applied with `denoise`)."""

    report = None

    def __init__(self, ref_audio, target_rms=0.1, device=None, denoise=False, reject_marked=None, assess=False, limits=None):
        wav, sr = ref_audio if isinstance(ref_audio, tuple) else load_audio(ref_audio)
        if denoise:
            check_denoise_length(resampled_length(wav.shape[-1], sr, target_sample_rate))
        self.seconds = wav.shape[-1] / sr
        self.audio, self.rms = _prepare_reference(wav, sr, target_rms, device)
        self.denoise = bool(denoise)
        self.limits = check_reference_limits(limits)
        self.assess = bool(assess) or self.limits is not None
        if self.assess:
            self.report = _assess_host(wav, sr, self.audio, self.rms)
            check_within_limits(self.report, self.limits, self.denoise)
        self.reject_marked = None if reject_marked is None else tuple(check_watermark_keys(list(reject_marked)))
        if self.reject_marked is not None:
            check_unmarked(self.audio, self.reject_marked)
        if self.denoise:
            self.audio = _denoise_host(self.audio)
        self.ref_frames = self.audio.shape[-1] // hop_length
        self.mel = None
        self.pending = None

    @classmethod
    def deferred(cls, ref_audio, target_rms=0.1, denoise=False, reject_marked=None, assess=False, limits=None):
        wav, sr = ref_audio
        if wav.dim() != 2 or wav.shape[-1] < 1:
            raise ValueError(f"reference audio must be [channels, samples] with at least one sample (got {tuple(wav.shape)})")
        if sr != target_sample_rate:
            resample_taps(sr, target_sample_rate)   # an unsupported rate pair is refused here, before anything is queued
        if denoise:
            check_denoise_length(resampled_length(wav.shape[-1], sr, target_sample_rate))
        voice = cls.__new__(cls)
        voice.denoise = bool(denoise)
        voice.limits = check_reference_limits(limits)
        voice.assess = bool(assess) or voice.limits is not None
        voice.reject_marked = None if reject_marked is None else tuple(check_watermark_keys(list(reject_marked)))
        voice.seconds = wav.shape[-1] / sr
        voice.ref_frames = resampled_length(wav.shape[-1], sr, target_sample_rate) // hop_length
        voice.audio = voice.rms = voice.mel = None
        voice.pending = (wav, int(sr), target_rms)
        return voice

    def cond(self, model_obj):
        """What to hand the sampler as the prompt: the cached mel [1, n, mel] when the model object can compute one, else the wave."""
        if self.pending is not None:
            _prepare_deferred([self], model_obj)
        if not hasattr(model_obj, "cond_mel"):
            return self.audio
        if self.mel is None:
            self.mel = model_obj.cond_mel(self.audio)
        return self.mel


# How often `prepare_voices` denoised: "host_clips" (one `denoise_reference` each) and "device_calls" (one `ops.ref_denoise` each, whatever
# the number of flagged voices in it).  A batch without a flagged voice adds to neither.
DENOISE_COUNTS = collections.Counter()


# How often reference clips were scored against `reject_marked` keys: "host_clips" (one `detect_watermark` each) and "device_calls" (one
# `ops.watermark_detect` each, whatever the number of clips and keys in it)
WATERMARK_COUNTS = collections.Counter()
MARKED_REFERENCE = "the reference clip carries this service's watermark"


def check_unmarked(audio, keys):
    """Refuses (ValueError, `MARKED_REFERENCE`: it names no key) a prepared 24 kHz wave [1, nw] that `detect_watermark` finds marked with any
    of `keys`, on the host."""
    WATERMARK_COUNTS["host_clips"] += 1
    if any(score.detected for score in detect_watermark(audio[0].detach().cpu().numpy(), list(keys))):
        raise ValueError(MARKED_REFERENCE)


# How often reference clips were measured: "host_clips" (one `assess_reference` each) and "device_calls" (one `ops.ref_assess` each, whatever
# the number of clips in it).  Without a voice that asks for a report neither moves.
ASSESS_COUNTS = collections.Counter()


def _assess_host(wav, sr, audio, rms):
    """`audio_prep.assess_reference` of a clip [ch, n] at `sr` and its prepared wave [1, nw], on the host."""
    ASSESS_COUNTS["host_clips"] += 1
    return assess_reference(wav.detach().cpu().to(torch.float32).numpy(), sr, audio[0].detach().cpu().numpy(), rms=float(rms))


def check_within_limits(report, limits, denoise=False):
    """Refuses (ValueError naming each violated measure, its value and the limit) a clip whose `report` violates `limits`."""
    problems = reference_problems(report, limits, denoise)
    if problems:
        raise ValueError("; ".join(problems))


def _denoise_host(audio):
    """`audio_prep.denoise_reference` of a prepared wave [1, nw], back where it was."""
    DENOISE_COUNTS["host_clips"] += 1
    return torch.from_numpy(denoise_reference(audio[0].detach().cpu().numpy()))[None].to(audio.device)


def prepare_voices(clips, target_rms=0.1, device="cuda"):
    """The reference-audio front-end (mono mix, rms, gain, resampling to 24 kHz) of several voices at once on the device: one upload of the
    packed clips and ONE `ops.ref_frontend` call (two launches) per distinct sample rate, then one download of all rms values.
    `clips` = [(wave [ch, n] fp32, sr)] -> [PreparedVoice], or deferred `PreparedVoice`s, which are filled in place (and returned).
    The mel stays lazy here (`cond`), one call per clip; a model object with `cond_mel_ragged` (`F5HipModel.prepare_voices`) fills the mel of
    every voice this call prepared in one launch behind it.  `device=None` runs the host `_prepare_reference` clip by clip instead (what a model
    object without the device front-end gets: the reference's modules, CPU stand-ins) and leaves the result on the host, like the eager
    constructor does.  Voices with `denoise` set are denoised behind the front-end: on the device the flagged voices of each front-end call
    -- one per distinct (sample rate, rms floor) -- go through ONE `ops.ref_denoise` on that call's packed output, in place, so a voice's
    `audio` view and the mel launch behind it see the denoised samples with no copy; a call without a flagged voice is followed by none.
    With `device=None` the host `denoise_reference` runs clip by clip.  Voices with `reject_marked` keys are scored in front of the denoiser:
    the flagged voices of a front-end call in ONE `ops.watermark_detect` call on its packed output against the union of their keys, of which
    only the score rows come down; a voice that carries one of its own keys is a ValueError (`MARKED_REFERENCE`) and the call's voices stay
    deferred.  With `device=None` `check_unmarked` runs clip by clip.  Voices with `assess` are measured first of all: those of a front-end
    call in ONE `ops.ref_assess` call on the call's two buffers (the packed upload and the packed output), of which only the rows come down;
    a voice that violates one of its `limits` is a ValueError and the call's voices stay deferred.  With `device=None`
    `audio_prep.assess_reference` runs clip by clip."""
    voices = [c if isinstance(c, PreparedVoice) else PreparedVoice.deferred(c, target_rms) for c in clips]
    todo = [v for v in voices if v.pending is not None]
    if device is None:
        for v in todo:
            wav, sr, floor = v.pending
            audio, rms = _prepare_reference(wav, sr, floor, None)
            if getattr(v, "assess", False):
                report = _assess_host(wav, sr, audio, rms)
                check_within_limits(report, v.limits, getattr(v, "denoise", False))
                v.report = report
            if getattr(v, "reject_marked", None) is not None:
                check_unmarked(audio, v.reject_marked)
            v.audio, v.rms = audio, rms
            if getattr(v, "denoise", False):
                v.audio = _denoise_host(v.audio)
            v.pending = None
        return voices
    from . import ops
    groups = {}
    for v in todo:
        groups.setdefault((v.pending[1], float(v.pending[2])), []).append(v)
    done = []
    for (sr, floor), vs in groups.items():
        packed = torch.cat([v.pending[0].to(torch.float32).reshape(-1) for v in vs]).to(device)
        taps = None if sr == target_sample_rate else _device_taps(sr, target_sample_rate, packed.device)
        out, rms, n_out = ops.ref_frontend(packed, [v.pending[0].shape[-1] for v in vs], [v.pending[0].shape[0] for v in vs], sr,
                                           target_sample_rate, taps, floor)
        starts = np.concatenate([[0], np.cumsum(n_out)[:-1]])
        measured = [i for i, v in enumerate(vs) if getattr(v, "assess", False) and n_out[i] > 0]
        reports = {}
        if measured:                                             # in front of the watermark check and the denoiser; only the rows come down
            sizes = [int(v.pending[0].shape[0]) * int(v.pending[0].shape[-1]) for v in vs]
            raw_at = np.concatenate([[0], np.cumsum(sizes)[:-1]])
            rows = ops.ref_assess(packed, [int(raw_at[i]) for i in measured], [int(vs[i].pending[0].shape[0]) for i in measured],
                                  [int(vs[i].pending[0].shape[-1]) for i in measured], out, [int(starts[i]) for i in measured],
                                  [min(int(n_out[i]), ASSESS_MAX_SAMPLES) for i in measured]).cpu().numpy()
            ASSESS_COUNTS["device_calls"] += 1
            for i, row in zip(measured, rows):
                reports[i] = report_from_row(row, vs[i].seconds, None, sizes[i])
                check_within_limits(reports[i], vs[i].limits, getattr(vs[i], "denoise", False))
        guarded = [i for i, v in enumerate(vs) if getattr(v, "reject_marked", None) is not None and n_out[i] > 0]
        if guarded:                                              # in front of the denoiser; only the score rows come down
            keys = sorted({k for i in guarded for k in vs[i].reject_marked})
            if len(keys) > WATERMARK_KEYS_MAX:
                raise ValueError(f"the voices of one front-end call name {len(keys)} watermark keys to reject; at most {WATERMARK_KEYS_MAX} in a call")
            rows = ops.watermark_detect(out, [int(starts[i]) for i in guarded], [min(int(n_out[i]), WATERMARK_MAX_SAMPLES) for i in guarded],
                                        ops.watermark_carriers(keys, out.device)).cpu().numpy()
            WATERMARK_COUNTS["device_calls"] += 1
            for i, row in zip(guarded, rows):
                if any(score.detected and score.key in vs[i].reject_marked for score in ops.watermark_scores(row, keys)):
                    raise ValueError(MARKED_REFERENCE)
        flagged = [i for i, v in enumerate(vs) if getattr(v, "denoise", False)]
        if flagged:                                              # in place on the packed output: the views below are the denoised clips
            ops.ref_denoise(out, [int(starts[i]) for i in flagged], [int(n_out[i]) for i in flagged])
            DENOISE_COUNTS["device_calls"] += 1
        done.append((vs, out.split(n_out), rms, reports))
    if done:
        all_rms = torch.cat([rms for _, _, rms, _ in done]).cpu()   # the one download
        k = 0
        for vs, outs, _, reports in done:
            for i, (v, audio) in enumerate(zip(vs, outs)):
                v.audio, v.rms, v.pending = audio[None], all_rms[k], None
                if i in reports:
                    v.report = reports[i]._replace(rms=float(all_rms[k]))
                k += 1
    return voices


def _prepare_deferred(voices, model_obj):
    """The deferred voices among `voices` (each once) through the model object's `prepare_voices` (F5HipModel, ShardedSampler: the device
    front-end, one ragged call), or through the host front-end when it has none."""
    todo = list({id(v): v for v in voices if v.pending is not None}.values())
    if not todo:
        return
    if hasattr(model_obj, "prepare_voices"):
        model_obj.prepare_voices(todo)
    else:
        prepare_voices(todo, device=None)


def _plan_request(ref_audio, ref_text, gen_text, target_rms, speed, fix_duration, device, tokenizer):
    """Host prologue of infer_batch_process for one request (F/infer/utils_infer.py:423-454): prepared reference wave, its rms,
    the frame count the reference strips afterwards, and one sampling unit per text chunk.  `gen_text`: a list of chunk texts used as
    they are, or a string chunked like `infer_process` does (`request_chunks`)."""
    voice = ref_audio if isinstance(ref_audio, PreparedVoice) else PreparedVoice(ref_audio, target_rms, device)
    chunks = list(gen_text) if isinstance(gen_text, (list, tuple)) else request_chunks(ref_text, voice.seconds, gen_text)
    if len(ref_text[-1].encode("utf-8")) == 1:
        ref_text = ref_text + " "
    return voice, plan_units(ref_text, chunks, voice.ref_frames, speed, fix_duration, tokenizer)


def request_generator(seed):
    """The CPU generator a request with `seed` draws its noise from: chunk k takes `randn(dur_k, mel)` after the draws of chunks 0..k-1, so
    chunks get different noise and the global generator is not touched.  None without a seed."""
    if seed is None:
        return None
    return torch.Generator().manual_seed(int(seed))


def _sample_units(model_obj, cond, audios, units, steps, cfg_strength, sway_sampling_coef, generators, ode_method=None):
    """The mels [frames_i, mel] (reference frames included) of `units`: ONE `sample_units` call when the model object offers it (`cond`: the
    prompts, one tensor for all units or one per unit; `generators`, one or None per unit, is handed on only when a unit has one), else the
    reference's batch-1 `.sample()` unit by unit on the waves `audios`.  Each knob: one value or one per unit.  `ode_method` (one name, or
    one name or None per unit) is handed on only when a unit names a solver."""
    methods = ode_method if isinstance(ode_method, list) else [ode_method] * len(units)
    if hasattr(model_obj, "sample_units"):
        extra = dict(generators=list(generators)) if any(g is not None for g in generators) else {}
        if any(name is not None for name in methods):
            extra["ode_method"] = ode_method
        return model_obj.sample_units(cond, units, steps=steps, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, **extra)
    if any(g is not None for g in generators):
        raise ValueError("a per-request seed needs a model object with sample_units (F5HipModel, ShardedSampler)")
    per_unit = [v if isinstance(v, list) else [v] * len(units) for v in (steps, cfg_strength, sway_sampling_coef)]
    return [model_obj.sample(cond=audio, text=[tokens], duration=frames, steps=n, cfg_strength=cfg, sway_sampling_coef=sway,
                             **({} if name is None else dict(ode_method=name)))[0][0]
            for audio, (tokens, frames), n, cfg, sway, name in zip(audios, units, *per_unit, methods)]


def _sample(model_obj, voice, units, knobs, generator=None):
    """`_sample_units` for one request's units: one shared prompt, one set of knobs.  `generator`: the request's own noise source
    (`request_generator`)."""
    return _sample_units(model_obj, voice.cond(model_obj), [voice.audio] * len(units), units, generators=[generator] * len(units), **knobs)


def _chunk_waves(groups, vocoder, mel_spec_type, target_rms, on_device=False, want_specs=True):
    """Vocoder part of infer_batch_process's tail (F/infer/utils_infer.py:468-481) for the chunks of several requests: `groups` =
    [(mels, ref_frames, rms)] -> per group ([wave_i], [spec_i]) as numpy, the reference frames stripped and the rms restored per chunk.
    `on_device`: the waves stay where the vocoder left them, as 1-D tensors (views of `decode_ragged`'s packed output where no gain applies),
    for `finish_requests`; `want_specs=False`: no spectrogram is downloaded and `[spec_i]` is None (the serving path drops them).
    Vocoder objects that offer `decode_ragged` vocode every chunk of every group in ONE call (each item equals its own `decode` /
    `vocoder(spec)`, bit for bit): F5HipVocos for "vocos", and for "bigvgan" an object whose `decode_ragged` is the BigVGAN one, which it
    says with `ragged_mel_spec_type == "bigvgan"` (F5HipBigVGAN; a Vocos-style `decode_ragged` returns hop (T - 1) samples per item, so
    the method's name alone does not make it usable here).  Any other vocoder (the reference's modules) is called chunk by chunk at batch 1
    like the reference, and so is a single BigVGAN chunk."""
    if mel_spec_type not in ("vocos", "bigvgan"):
        raise ValueError(mel_spec_type)
    specs = [[mel.to(torch.float32)[ref_frames:, :].t()[None] for mel in mels] for mels, ref_frames, _ in groups]   # [1, mel, T] (:468-470)
    flat = [spec for g in specs for spec in g]
    if mel_spec_type == "vocos":
        ragged = hasattr(vocoder, "decode_ragged") and len(flat) > 0
    else:
        # A single chunk (a streamed request's head, a span boundary with one ticket) takes the plain forward: the ragged call runs the same
        # kernels for it and adds the slab copy, the length tables and their upload, so at n = 1 it can only match or lose
        ragged = hasattr(vocoder, "decode_ragged") and getattr(vocoder, "ragged_mel_spec_type", None) == "bigvgan" and len(flat) > 1
    if ragged:
        # shaped like `decode(spec)` [1, n] resp. `vocoder(spec)` [1, 1, n]
        raw = [w[None] if mel_spec_type == "vocos" else w[None, None] for w in vocoder.decode_ragged([spec[0] for spec in flat])]
    else:
        raw = [vocoder.decode(spec) if mel_spec_type == "vocos" else vocoder(spec) for spec in flat]
    out, k = [], 0
    for (_, _, rms), g in zip(groups, specs):
        waves = []
        for wave in raw[k:k + len(g)]:
            if rms < target_rms:
                wave = wave * rms / target_rms
            if on_device:
                waves.append(wave.reshape(-1))
            else:
                waves.append(wave.squeeze().cpu().numpy())
                backend_stats["d2h_copies"] += int(wave.is_cuda)
        out.append((waves, [spec[0].cpu().numpy() for spec in g] if want_specs else None))
        backend_stats["d2h_copies"] += sum(int(spec.is_cuda) for spec in g) if want_specs else 0
        k += len(g)
    return out


def _vocode_and_join(mels, ref_frames, rms, vocoder, mel_spec_type, target_rms, cross_fade_duration):
    """Tail of infer_batch_process (F/infer/utils_infer.py:468-524): strip the reference frames, vocode, restore the rms, cross-fade."""
    (waves, specs), = _chunk_waves([(mels, ref_frames, rms)], vocoder, mel_spec_type, target_rms)
    return cross_fade_concat(waves, cross_fade_duration), target_sample_rate, np.concatenate(specs, axis=1)


def infer_batch_process(ref_audio, ref_text, gen_text_batches, model_obj, vocoder, mel_spec_type="vocos", progress=None,
                        target_rms=0.1, cross_fade_duration=0.15, nfe_step=32, cfg_strength=2.0, sway_sampling_coef=-1,
                        speed=1, fix_duration=None, device=None, tokenizer=text_to_tokens, seed=None, ode_method=None):
    """F/infer/utils_infer.py:406-524, same signature and return triple.

    The reference loops over the chunks and calls `sample()` / the vocoder once per chunk with batch 1.  The chunks are independent
    units, so here they are planned first and sampled in ONE `sample_units()` call when the model object offers it (F5HipModel: all
    chunks packed back to back, each with the reference's batch-1 semantics, the reference-audio mel computed once instead of once
    per chunk); any other object with the reference's `.sample()` is driven chunk by chunk like the reference does."""
    voice, units = _plan_request(ref_audio, ref_text, gen_text_batches, target_rms, speed, fix_duration, device, tokenizer)
    knobs = dict(steps=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, ode_method=ode_method)
    mels = _sample(model_obj, voice, units, knobs, request_generator(seed))   # list of [frames_i, mel] incl. the reference frames
    return _vocode_and_join(mels, voice.ref_frames, voice.rms, vocoder, mel_spec_type, target_rms, cross_fade_duration)


# per-request options of `infer_requests` (the fourth element of a request) and of the serving routes
REQUEST_OPTIONS = ("speed", "nfe_step", "cfg_strength", "sway_sampling_coef", "seed", "ode_method", "remove_silence", "sample_rate", "encoding",
                   "loudness", "flac_level") + WATERMARK_OPTIONS + FORMANT_OPTIONS + PROSODY_OPTIONS   # the sampler's six, then the nine of
#                                            `WaveSpec` (`WAVE_OPTIONS`): `DELIVERY_OPTIONS`, `watermark`, `keep_formants` and `PROSODY_OPTIONS`


def needs_whole_wave(opts, streamed=False) -> bool:
    """`WaveSpec.needs_whole_wave` of a dict of options: whether the request cannot be handed out chunk by chunk (`WHOLE_WAVE`)."""
    return WaveSpec.of(opts).needs_whole_wave(streamed)


def whole_wave_message(opts) -> str:
    """`WaveSpec.whole_wave_message` of a dict of options."""
    return WaveSpec.of(opts).whole_wave_message()


def plan_request(request, defaults, *, target_rms, fix_duration, device, tokenizer):
    """One request tuple (ref_audio, ref_text, gen_text[, options]) of `infer_requests` / `SpanScheduler.admit`, planned: `opts` (the
    options over `defaults`, unknown ones rejected), `spec` (`WaveSpec.of(opts)`: what the finished wave has to be, its mark and `keep_formants` included), `voice` (prepared),
    `units` (one per chunk; the text is chunked unless it is a list of chunk texts) and `generator`, the request's noise source (None: the
    global one).  A `ScriptRequest` is planned segment by segment:
    `parts` = [(voice, units)] per segment (a plain request has one part), `units` all of them in order -- one generator, so chunk k of the
    script draws after chunks 0..k-1 of the whole script -- `voice` the first segment's, `script` the request itself (None: a tuple).  A `generator` the request carries is drawn from
    on a copy: `commit()` moves the caller's to where the copy got, once the caller knows that the request went through."""
    script = request if isinstance(request, ScriptRequest) else None
    own_opts = script.options if script is not None else (request[3] if len(request) > 3 and request[3] else {})
    opts = dict(defaults, **own_opts)
    unknown = set(opts) - set(REQUEST_OPTIONS) - {"generator"}
    if unknown:
        raise ValueError(f"unknown request option(s) {sorted(unknown)}; known: {list(REQUEST_OPTIONS)}")
    spec = WaveSpec.of(opts)
    if spec.needs_whole_wave() and isinstance(request_text(request), (list, tuple)):
        raise ValueError(spec.whole_wave_message())
    # one (voice, units) part per segment; a plain request is its own single segment
    segments = script.segments if script is not None else [tuple(request[:3])]
    parts = [_plan_request(seg[0], seg[1], seg[2], target_rms, seg[3] if len(seg) > 3 and seg[3] is not None else opts["speed"], fix_duration,
                           device, tokenizer) for seg in segments]
    voice, units = parts[0][0], [u for _, us in parts for u in us]
    own = opts.get("generator")
    gen = torch.Generator().set_state(own.get_state()) if own is not None else request_generator(opts["seed"])

    def commit():
        if own is not None:
            own.set_state(gen.get_state())
    return types.SimpleNamespace(voice=voice, units=units, opts=opts, spec=spec, generator=gen, commit=commit, parts=parts, script=script)


def infer_requests(requests, model_obj, vocoder, mel_spec_type=mel_spec_type, target_rms=target_rms,
                   cross_fade_duration=cross_fade_duration, nfe_step=nfe_step, cfg_strength=cfg_strength,
                   sway_sampling_coef=sway_sampling_coef, speed=speed, fix_duration=fix_duration, device=None, tokenizer=text_to_tokens,
                   join=True, finish=None):
    """Several `infer_process()` calls as ONE sampler batch: `requests` = [(ref_audio, ref_text, gen_text)], each with its own
    reference voice (a path, a (wave, sr) pair or a `PreparedVoice`); returns one (wave, sample_rate, spectrogram) triple per request, each what `infer_process` returns for
    that request alone: units keep the reference's batch-1 semantics (no padding against each other, no shared mask), and noise is drawn
    unit by unit in request order, i.e. the draws of the sequential calls.  Bit for bit this holds when the model handle runs the
    shape-invariant attention arithmetic (`F5HipModel(attn_shape_invariant=True)`, what `serve.TTSManager.load` sets); in the default
    mode a lone unit and the same unit inside a batch may take different attention kernels (same values to the last bits per launch, but
    in the mixed GEMM mode last-bit differences grow to that mode's rounding-noise floor, 4.4e-4 rms after two Euler steps:
    `profiles/r03_attn_mode_tapdiff.txt`; either result is within the 1e-3 bound of the reference).  This is what the serving queue (`serve.MicroBatcher`) and the
    multi-voice front-end hand to the GPU: the chunks of all waiting requests are packed back to back in one library call, and with a
    vocoder object that offers `decode_ragged` (F5HipVocos, F5HipBigVGAN) they are vocoded in one call too.

    `gen_text` is a string, chunked like `infer_process` does, or a list of chunk texts used as they are (a streamed request's first
    chunk and its remaining chunks ride in different batches: `infer_process_stream`, `serve.TTSManager.synthesize_stream`).  Unseeded,
    such a request draws its remaining chunks' noise one batch later than it would unstreamed, so under concurrency its result is a
    different valid sample; alone, or with the generator reseeded, it is the same.  `join=False` returns ([wave_i], sample_rate,
    [spec_i]) per request -- the per-chunk waves before the cross-fade -- instead of the joined triple.

    Per-request options: a request may carry a fourth element, a dict with any of `speed`, `nfe_step`, `cfg_strength`,
    `sway_sampling_coef`, `seed` and `ode_method` (`REQUEST_OPTIONS`); what it leaves out comes from this function's keyword arguments
    (`ode_method`: from the model object, which is handed the option only for requests that set it).  With a model
    that declares `per_unit_time_grids` (`F5HipModel`: f5hip_cfm_sample_grids) all units are sampled in ONE `sample_units` call whatever
    their time grids (`nfe_step`, `sway_sampling_coef`), strengths and solvers: each knob goes in as one value when all units agree, else as
    one value per unit.  With any other model, requests that share a time grid are sampled in one call and each further grid is one more call,
    in order of first appearance.  All chunks are vocoded together either way.  `speed` only changes a request's planned frames.  With `seed`, the request's chunk k draws its noise from `request_generator(seed)` after chunks
    0..k-1; a `generator` entry (a torch.Generator) continues that sequence instead -- what a streamed request's remaining chunks carry --
    and is advanced only when this call succeeds.  A seeded request's result depends only on its own settings, not on its batch, with the
    shape-invariant attention mode on one GPU (ranks > 0 of a `serve.ShardedSampler` do not switch to that mode yet); unseeded units draw
    from the global generator in flat request order (unit by unit, request after request) when there is one sampler call, i.e. always
    with a `per_unit_time_grids` model, and in sampler-call order otherwise.

    The `DELIVERY_OPTIONS` (`remove_silence`, `loudness`, `sample_rate`, `encoding`, `flac_level`), per request, say what its finished wave
    is, and the `PROSODY_OPTIONS` (`tempo`, `pitch`) move its duration and pitch behind the model (`shift_pcm16`, where `speed` asks the
    sampler for another take): see `WaveSpec`.  Such a request's wave is `finish_pcm16` of its quantised joined wave and its triple names the delivery rate; the
    ones that need the whole wave are a ValueError with `join=False` or a list of chunk texts.  A `ScriptRequest` (a multi-voice script:
    one segment per piece, each with its own voice) is accepted in place of a tuple: its
    segments' units ride in the same sampler call, one prompt per unit, and the same vocoder call, one group per segment; its triple is
    (`join_segments` of its segments' chunk waves, rate, [spectrogram per segment]), with `join=False` the chunk waves and spectrograms per
    segment, and its whole-wave options apply to the joined script.  `finish` = dict(device_backend=..., want=...): what the serving path asks for -- the list of `finish_requests`
    results (one wave per request, no triples) with no spectrogram downloaded."""
    defaults = dict(speed=speed, nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=None)
    calls = {}   # calls: (nfe_step, sway, ode_method) -> [unit ids, ...] of one sampler call each
    flat_units, flat_cond, flat_audio, flat_cfg, flat_gen, flat_grid = [], [], [], [], [], []
    plans = [plan_request(req, defaults, target_rms=target_rms, fix_duration=fix_duration, device=device, tokenizer=tokenizer) for req in requests]
    _prepare_deferred([voice for plan in plans for voice, _ in plan.parts], model_obj)   # uploaded clips: one ragged front-end call for all of them
    for plan in plans:
        opts = plan.opts
        key = (int(opts["nfe_step"]), opts["sway_sampling_coef"], opts.get("ode_method"))
        for voice, units in plan.parts:   # (a script: its segments one after the other, each unit with its own voice's prompt)
            calls.setdefault(key, []).extend(range(len(flat_units), len(flat_units) + len(units)))
            flat_units += units
            flat_cond += [voice.cond(model_obj)] * len(units)
            flat_audio += [voice.audio] * len(units)
            flat_cfg += [opts["cfg_strength"]] * len(units)
            flat_gen += [plan.generator] * len(units)
            flat_grid += [key] * len(units)
    if len(calls) > 1 and getattr(model_obj, "per_unit_time_grids", False):
        calls = {None: list(range(len(flat_units)))}   # one call for every grid
    mels = [None] * len(flat_units)

    def one_or_list(vals):
        return vals[0] if all(v == vals[0] for v in vals) else vals

    for ids in calls.values():
        got = _sample_units(model_obj, [flat_cond[i] for i in ids], [flat_audio[i] for i in ids], [flat_units[i] for i in ids],
                            one_or_list([flat_grid[i][0] for i in ids]), one_or_list([flat_cfg[i] for i in ids]),
                            one_or_list([flat_grid[i][1] for i in ids]), [flat_gen[i] for i in ids], one_or_list([flat_grid[i][2] for i in ids]))
        for i, mel in zip(ids, got):
            mels[i] = mel
    groups, k = [], 0
    for plan in plans:
        plan.commit()   # every sampler call went through: the caller's generator moves
        for voice, units in plan.parts:   # one group per segment: each voice's rms is restored on its own chunks
            groups.append((mels[k:k + len(units)], voice.ref_frames, voice.rms))
            k += len(units)
    per_plan = np.cumsum([0] + [len(plan.parts) for plan in plans])   # a plan's groups: [per_plan[i], per_plan[i + 1])
    if finish is not None:
        backend = bool(finish.get("device_backend"))
        got = _chunk_waves(groups, vocoder, mel_spec_type, target_rms, on_device=backend, want_specs=False)
        chunk_waves = [request_chunk_waves(plan, got[per_plan[i]:per_plan[i + 1]]) for i, plan in enumerate(plans)]
        return _finish_specs(chunk_waves, [request_text(req) for req in requests], cross_fade_duration, [plan.spec for plan in plans], **finish)
    refused = next((plan for plan in plans if plan.spec.needs_whole_wave()), None)
    if refused is not None and not join:
        raise ValueError(refused.spec.whole_wave_message())
    out = []
    got = _chunk_waves(groups, vocoder, mel_spec_type, target_rms)
    for i, plan in enumerate(plans):
        mine, script = got[per_plan[i]:per_plan[i + 1]], plan.script is not None
        if join:   # a script: (wave, rate, [spectrogram per segment]) like `infer_multi_voice`
            joined_specs = [np.concatenate(specs, axis=1) for _, specs in mine]
            if script or plan.spec.needs_whole_wave():
                wave, = _finish_specs([request_chunk_waves(plan, mine)], [""], cross_fade_duration, [plan.spec])
            else:
                wave = cross_fade_concat(mine[0][0], cross_fade_duration)
            out.append((wave, plan.spec.sample_rate, joined_specs if script else joined_specs[0]))
        elif script:   # join=False: the chunk waves and spectrograms per segment
            out.append(([waves for waves, _ in mine], target_sample_rate, [specs for _, specs in mine]))
        else:
            out.append((mine[0][0], target_sample_rate, mine[0][1]))
    return out


def request_wave(gen_text, waves, cross_fade_duration=cross_fade_duration):
    """What a served request gets for its chunk waves: the per-chunk waves themselves when its text was a list of chunk texts (a streamed
    request's head or tail, joined by the caller's `StreamJoiner`), else the joined wave as float32."""
    if isinstance(gen_text, (list, tuple)):
        return waves
    return np.asarray(cross_fade_concat(waves, cross_fade_duration), dtype=np.float32)


# What `finish_requests` and `_chunk_waves` did since the last `backend_stats.clear()`: requests finished on the device / on the host,
# `ops.wave_finish` calls, `ops.wave_encode` calls and the requests they encoded (`encode_calls`, `encode_requests`), and device-to-host copies
# (chunk waves, spectrograms, PCM, encoded samples, lengths); `flac_bytes` is the size of the FLAC stream downloads; `loudness_calls` /
# `loudness_requests`: `ops.wave_loudness` calls and the requests they normalised; `prosody_calls` / `prosody_requests`: `ops.wave_prosody`
# calls and the requests whose tempo or pitch they changed; `mark_calls` / `mark_requests`: `ops.wave_mark` calls and the requests they marked
backend_stats: collections.Counter = collections.Counter()


def _host_chunk(wave):
    """A chunk wave as numpy, downloaded (and counted) when `_chunk_waves(on_device=True)` left it on the device."""
    if torch.is_tensor(wave):
        backend_stats["d2h_copies"] += int(wave.is_cuda)
        return wave.cpu().numpy()
    return wave


def _per_request(value, n, what):
    vals = list(value) if isinstance(value, (list, tuple)) else [value] * n
    if len(vals) != n:
        raise ValueError(f"finish_requests: one {what} or one per request ({n}), got {len(vals)}")
    return vals


def finish_requests(chunk_waves_per_request, gen_texts, cross_fade_duration=cross_fade_duration, remove_silence=None, device_backend=False,
                    want="float", sample_rate=None, encoding=None, loudness=None, flac_level=None, tempo=None, pitch=None, watermark=None,
                    keep_formants=None):
    """From the chunk waves of several requests (rms restored; numpy, or tensors as `_chunk_waves(on_device=True)` leaves them) to what each
    request gets.  A request whose text is a list of chunk texts (a streamed request's head or tail) gets its chunk waves as they are, like
    `request_wave`; a script's (`SegmentedWaves`: one list of chunk waves per segment) as one list per segment.  Any other request gets its
    joined wave -- `join_segments` for a script, which is eligible for the device call when every chunk is at least as long as the fades it
    takes part in (`_script_on_device`) and then rides in the same single call, `ops.wave_finish_joins` --: float32 (`request_wave`) with want="float", int16 PCM (`quantise_pcm16` of that)
    with want="pcm16" -- and, with its `remove_silence` flag set, `audio_prep.remove_silence_pcm` of that PCM whatever `want` says.

    `device_backend=True` (needs want="pcm16") makes ONE `ops.wave_finish` call for all eligible requests of the batch -- join, quantisation
    and silence removal on the device, bit for bit the host arithmetic -- and then at most two device-to-host copies: the lengths (only when
    a request asked for silence removal) and the samples.  Not eligible, and finished on the host in the same call (counted in
    `backend_stats`): a list text, chunk waves that are not on a HIP device, and a request of several chunks with one shorter than twice the
    fade, where the reference's nested cross-fades overlap and the kernel's closed form does not hold.

    `sample_rate` / `encoding`, `loudness`, `flac_level`, `tempo`, `pitch`, `watermark`, `keep_formants`: each one value or one per request, None for the
    default; with the flag they are the request's `WaveSpec` (one `WaveSpec.of` per request, so of several bad requests the first one
    reports), and a request that sets any of them gets `finish_pcm16` of its int16 PCM (quantised whatever `want` says).
    `watermark`: one key or one per request (`check_watermark`; None: no mark): the request's PCM gets `mark_pcm16`
    between the prosody and the loudness steps.  In the place of a key a `WatermarkTag(key, id)` (or `{"key": K, "id": I}`) makes the mark
    carry the request's trace id too (`read_watermark` reads it back): still one mark call for the batch, tagged and untagged together.
    `keep_formants`: one bool or one per request (`check_keep_formants`; None: no): with it the request's
    `pitch` keeps the spectral envelope (`shift_pcm16(..., keep_formants=True)`); without a pitch it is refused.
    With `device_backend` all of it stays on the device, chained on one stream behind `wave_finish`: the calls and the copies that come back
    are `_finish_on_device`'s, and `backend_stats` counts them."""
    _check_want(device_backend, want)   # (first, as ever: a bad `want` is reported before a bad option)
    n = len(chunk_waves_per_request)
    flags = [False] * n if remove_silence is None else [bool(f) for f in remove_silence]
    if len(gen_texts) != n or len(flags) != n:
        raise ValueError("finish_requests: one text and one remove_silence flag per request")
    one = isinstance(watermark, (WatermarkTag, dict))   # (a tag is a tuple: one value, not one per request)
    keywords = dict(sample_rate=sample_rate, encoding=encoding, loudness=loudness, flac_level=flac_level, tempo=tempo, pitch=pitch,
                    watermark=[watermark] * n if one else watermark, keep_formants=keep_formants)
    columns = [_per_request(value, n, name) for name, value in keywords.items()]
    specs = [WaveSpec.of(dict(zip(keywords, row), remove_silence=flag)) for flag, *row in zip(flags, *columns)]
    return _finish_specs(chunk_waves_per_request, gen_texts, cross_fade_duration, specs, device_backend, want)


def _check_want(device_backend, want):
    if want not in ("float", "pcm16"):
        raise ValueError(f'want must be "float" or "pcm16" (got {want!r})')
    if device_backend and want != "pcm16":
        raise ValueError('the device back-end produces int16 PCM: device_backend=True needs want="pcm16"')


def _finish_specs(chunk_waves_per_request, gen_texts, cross_fade_duration, specs, device_backend=False, want="float"):
    """`finish_requests` with one planned `WaveSpec` per request in place of its option keywords: what `infer_requests` and `SpanScheduler` call."""
    _check_want(device_backend, want)
    fade = int(cross_fade_duration * target_sample_rate) if cross_fade_duration > 0 else 0
    out, on_device = [None] * len(specs), []
    for i, (waves, text, spec) in enumerate(zip(chunk_waves_per_request, gen_texts, specs)):
        script = isinstance(waves, SegmentedWaves)
        if isinstance(text, (list, tuple)):
            if spec.needs_whole_wave():
                raise ValueError(spec.whole_wave_message())
            out[i] = [[_host_chunk(w) for w in seg] for seg in waves] if script else [_host_chunk(w) for w in waves]
        elif script and device_backend and _script_on_device(waves, fade):
            on_device.append(i)
            continue
        elif not script and device_backend and all(torch.is_tensor(w) and w.is_cuda for w in waves) and (len(waves) == 1 or min(len(w) for w in waves) >= 2 * fade):
            on_device.append(i)
            continue
        else:
            out[i] = _finish_on_host(waves, text, cross_fade_duration, spec, want)
        backend_stats["host_requests"] += 1
    if on_device:
        # the plain requests first: their PCM is then one prefix of the packed buffer, and what comes down of it holds no other request's
        on_device.sort(key=lambda i: not specs[i].plain_format)
        done = _finish_on_device([_device_request(chunk_waves_per_request[i]) for i in on_device], fade, [specs[i] for i in on_device])
        for i, wave in zip(on_device, done):
            out[i] = wave
    return out


def _script_on_device(segments, fade):
    """Whether the device back-end takes a script's chunk waves: all on a HIP device, and every chunk at least as long as the fades it
    takes part in (`fade` if it fades into its predecessor, plus `fade` if its successor fades into it) -- where `join_segments`' nested
    cross-fades take `fade` samples that no other fade touched, which is the kernel's closed form."""
    if not all(torch.is_tensor(w) and w.is_cuda for seg in segments for w in seg):
        return False
    return all(len(w) >= (fade if c > 0 else 0) + (fade if c + 1 < len(seg) else 0) for seg in segments for c, w in enumerate(seg))


def _device_request(waves):
    """A request for `_finish_on_device`: (chunk waves, fades) -- `fades` None for a plain request (every join fades), else one bool per
    chunk: a segment's first chunk butts against what is in front of it, and so does a gap (a chunk of zeros) and what follows it."""
    if not isinstance(waves, SegmentedWaves):
        return list(waves), None
    chunks, fades = [], []
    for i, seg in enumerate(waves):
        if i and waves.gap_samples > 0:
            chunks.append(torch.zeros(waves.gap_samples, dtype=torch.float32, device=seg[0].device))
            fades.append(False)
        chunks += list(seg)
        fades += [False] + [True] * (len(seg) - 1)
    return chunks, fades


def finish_pcm16(pcm, spec) -> np.ndarray:
    """What a `WaveSpec` makes of a request's 24 kHz int16 PCM, the one
    host definition (the device back-end and `StreamDelivery` are held to it byte for byte): `remove_silence_pcm` when flagged,
    `shift_pcm16` (tempo and pitch; with `keep_formants` the pitch by `psola_pcm16`, which keeps the spectral envelope),
    `mark_pcm16` with a key -- so the loudness and the -1 dBFS peak cap are measured on the marked samples, and the one gain behind it does
    not disturb the scale-invariant detector --, `normalise_loudness_pcm16`, `deliver_pcm16`."""
    if spec.remove_silence:
        pcm = remove_silence_pcm(pcm, target_sample_rate)
    pcm = shift_pcm16(pcm, spec.tempo, spec.pitch, spec.keep_formants)
    pcm = mark_pcm16(pcm, spec.watermark)
    pcm = normalise_loudness_pcm16(pcm, spec.loudness)
    return deliver_pcm16(pcm, *spec.format, flac_level=spec.flac_level if spec.flac else None)


def _finish_on_host(waves, text, cross_fade_duration, spec, want):
    """`finish_requests` for one request on the host: join, quantisation where anything asks for PCM, `finish_pcm16`."""
    if isinstance(waves, SegmentedWaves):
        wave = join_segments([[_host_chunk(w) for w in seg] for seg in waves], cross_fade_duration, waves.gap_samples)
    else:
        wave = request_wave(text, [_host_chunk(w) for w in waves], cross_fade_duration)
    if spec.needs_whole_wave():
        return finish_pcm16(quantise_pcm16(wave), spec)
    return quantise_pcm16(wave) if want == "pcm16" else wave   # (nothing to finish: no pass through the three steps' own checks)


def _finish_on_device(requests, fade, specs):
    """`finish_requests` for the requests the device back-end takes: `requests` = (chunk waves (device tensors), fades: `_device_request`)
    and their `specs`, the plain-format ones first.  ONE `ops.wave_finish` call -- `ops.wave_finish_joins` when a script is among them --;
    directly behind it, when any request names a tempo or a pitch, ONE `ops.wave_prosody` call for the whole batch (the others are copied
    through), whose buffer, offsets, bounds and device lengths everything downstream reads in the place of `wave_finish`'s -- with a spec that
    has `keep_formants` the same ONE call, flagged and unflagged requests together: a flagged request takes the
    stretch of its tempo alone and keeps its spectral envelope (`backend_stats["formant_requests"]`);
    then, when any spec has a key or a `WatermarkTag` for its `watermark`, ONE `ops.wave_mark` call that marks
    those in place, with their trace ids where they have one (f5hip_wave_mark_ids then; the same two launches, no copy more)
    (carriers cached on the device: nothing is uploaded for a key seen before, and nothing comes back);
    then, when any request has a loudness target, ONE `ops.wave_loudness` call that normalises those in place; then on the
    same stream one `ops.wave_flac` call per distinct rate of the "flac" requests (behind a `wave_encode(..., "pcm16")` call where the rate
    is not 24 kHz; the requests of a rate share it through its per-request levels, and a call in which nobody asks for level 1 is the
    level-0 call) and one `ops.wave_encode` call per other distinct delivery format.  Every call is queued before the first copy comes
    back; a flagged request's length stays on the device in between.  Copies: the plain requests' lengths (only with silence removal) and
    samples; per `wave_encode` format the lengths (only with silence removal) and the encoded samples, nothing of the 24 kHz PCM; per
    FLAC rate the streams' lengths, then the streams, joined on the device, in one download of exactly their bytes; none for the loudness
    call.  Like every ragged call of the library each `wave_encode` call copies its small request table on the stream and waits for that
    copy before it launches, so the host does wait once per format for what is queued in front of it; no data comes back in that wait.
    Returns one result per request."""
    from . import ops
    out = [None] * len(requests)
    silence = [spec.remove_silence for spec in specs]
    plain = sum(spec.plain_format for spec in specs)
    chunks = [w.to(torch.float32).contiguous() for waves, _ in requests for w in waves]
    fades = [[False] + [True] * (len(waves) - 1) if f is None else f for waves, f in requests]
    joined = [sum(len(w) for w in waves) - sum(f[1:]) * fade for (waves, _), f in zip(requests, fades)]
    counts = [len(waves) for waves, _ in requests]
    if all(f is None for _, f in requests):
        pcm, lengths, offsets = ops.wave_finish(chunks, counts, fade, silence, target_sample_rate)
    else:
        pcm, lengths, offsets = ops.wave_finish_joins(chunks, counts, fade, [x for f in fades for x in f], silence, target_sample_rate)
    if any(spec.prosody for spec in specs):   # one call for the batch; lengths stay on the device, and `joined` becomes the new bounds
        keeps = [spec.keep_formants for spec in specs]
        flagged = {}   # (nobody flagged: the argument is left out, and the call is the older entry point with its launch count)
        if any(keeps):
            flagged = {"keep_formants": keeps}
            backend_stats["formant_requests"] += sum(keeps)
        pcm, lengths, offsets, joined = ops.wave_prosody(pcm, offsets, joined, lengths, [spec.stretch for spec in specs], [spec.pitch for spec in specs], **flagged)
        backend_stats["prosody_calls"] += 1
        backend_stats["prosody_requests"] += sum(spec.prosody for spec in specs)
    marks = [spec.watermark for spec in specs]
    if any(key is not None for key in marks):   # in place, lengths still on the device: nothing comes back for it
        ops.wave_mark(pcm, offsets, joined, lengths, marks)
        backend_stats["mark_calls"] += 1
        backend_stats["mark_requests"] += sum(key is not None for key in marks)
    targets = [spec.gain_constant for spec in specs]
    if any(t is not None for t in targets):   # in place, lengths still on the device: nothing comes back for it
        ops.wave_loudness(pcm, offsets, joined, lengths, targets)
        backend_stats["loudness_calls"] += 1
        backend_stats["loudness_requests"] += sum(t is not None for t in targets)
    if plain:
        if any(silence[:plain]):
            kept = lengths[:plain].cpu().tolist()
            backend_stats["d2h_copies"] += 1
        else:   # without silence removal a request keeps its joined length
            kept = joined[:plain]
        host = pcm[:offsets[plain - 1] + joined[plain - 1]].cpu().numpy()
        backend_stats["d2h_copies"] += 1
        for k, (off, length) in enumerate(zip(offsets, kept)):
            out[k] = host[off:off + length].copy()   # (a request's result does not keep the batch's buffer alive)
    groups = {}   # delivery format -> its requests, in order of first appearance: the "flac" requests of a rate are one group
    for k in range(plain, len(requests)):
        groups.setdefault(specs[k].format, []).append(k)

    def gathered(ks):   # the requests' lengths, gathered on the device
        contiguous = ks == list(range(ks[0], ks[-1] + 1))
        return lengths[ks[0]:ks[-1] + 1] if contiguous else lengths[torch.tensor(ks, device=lengths.device)]

    def encode(ks, rate, enc):   # one `ops.wave_encode` call, behind what is queued on the same stream
        taps = _device_taps(target_sample_rate, rate, pcm.device) if rate != target_sample_rate else None
        got = ops.wave_encode(pcm, [offsets[k] for k in ks], [joined[k] for k in ks], gathered(ks), rate, enc, taps)
        backend_stats["encode_calls"] += 1
        backend_stats["encode_requests"] += len(ks)
        return got

    # every group's kernels are queued first, the FLAC groups' in front, and only then does anything come down: a mixed micro-batch does not
    # wait for one group's copies before the next group's launches
    queued = []
    for (rate, enc), ks in sorted(groups.items(), key=lambda group: group[0][1] not in FLAC_ENCODINGS):
        if enc not in FLAC_ENCODINGS:
            queued.append((rate, enc, ks) + tuple(encode(ks, rate, enc)))
            continue
        if rate == target_sample_rate:   # one `ops.wave_flac` call per distinct rate, behind the resampler's where the rate is not 24 kHz
            src, src_off, sel = pcm, [offsets[k] for k in ks], gathered(ks)
        else:
            data, sel, out_off = encode(ks, rate, "pcm16")
            src, src_off = data.view(torch.int16), [off // 2 for off in out_off]
        levels = [specs[k].flac_level for k in ks]
        bounds = [resampled_length(joined[k], target_sample_rate, rate) for k in ks]
        queued.append((rate, enc, ks) + tuple(ops.wave_flac(src, src_off, bounds, sel, rate, level=levels if any(levels) else None)))
        backend_stats["flac_calls"] += 1
        backend_stats["flac_requests"] += len(ks)
    for rate, enc, ks, data, out_len, out_off in queued:
        flac = enc in FLAC_ENCODINGS
        if flac or any(silence[k] for k in ks):   # (a FLAC stream's length is known on the device alone)
            sizes = out_len.cpu().tolist()
            backend_stats["d2h_copies"] += 1
        else:
            sizes = [resampled_length(joined[k], target_sample_rate, rate) for k in ks]
        if flac:
            # `wave_flac` puts each stream at the offset its VERBATIM bound allows for, so between two streams lies room that nobody wrote:
            # the streams are joined on the device, and ONE download brings exactly their bytes and nothing of their PCM
            slices = [data[off:off + m] for off, m in zip(out_off, sizes)]
            # from here on `data` is the joined streams and `out_off` where each starts in them, so that the download and the split
            # below are the other formats' (a stream is uint8: one byte per unit of `sizes`)
            data, out_off = slices[0] if len(slices) == 1 else torch.cat(slices), np.cumsum([0] + sizes[:-1]).tolist()
            backend_stats["flac_bytes"] += sum(sizes)
        host = data.cpu().numpy()
        backend_stats["d2h_copies"] += 1
        for k, off, m in zip(ks, out_off, sizes):
            raw = host[off:off + m * (2 if enc == "pcm16" else 1)].copy()
            out[k] = raw.view("<i2") if enc == "pcm16" else raw
    backend_stats["device_calls"] += 1
    backend_stats["device_requests"] += len(requests)
    return out


class SpanTicket:
    """One admitted request of a `SpanScheduler`: its planned units, `spec` (`plan_request`'s `WaveSpec`: what the finished wave has to be),
    and -- once the units have all ended -- `result` (`request_wave`)."""

    def __init__(self, request, voice, units, spec, parts=None, script=None):
        self.request, self.voice, self.units, self.spec = request, voice, units, spec
        self.parts = parts if parts is not None else [(voice, units)]   # [(voice, its units)]: one per segment of a script
        self.script = script
        self.in_flight = self.cancelled = self.done = False
        self.result = None

    @property
    def frames(self) -> int:
        return sum(u.dur for u in self.units)

    def cancel(self):
        """Drops the request: its units leave at the next span boundary (nothing happens once it is done)."""
        self.cancelled = True


class SpanScheduler:
    """Continuous batching over resumable sampler spans, synchronous and without threads: `admit(request)` plans a request (as
    `infer_requests` plans it) and queues it; every `step()` is one span boundary followed by one span: cancelled tickets leave, waiting
    tickets join in order of arrival while they fit, all units in flight advance by `span_steps` ODE steps of their own grids in ONE
    `model_obj.advance` call (f5hip_cfm_sample_span; a unit whose request names an `ode_method` is budgeted in backbone forwards, `model.span_slices`), and the requests whose units have all ended are vocoded together (`_chunk_waves`:
    ragged Vocos when the vocoder offers it) and returned.  So a request waits for at most one span of the others, not for their whole
    batch, and with the shape-invariant attention mode its result is what `infer_requests` gives it alone with the same noise.

    Requests are `infer_requests`' tuples, per-request options included.  Noise is drawn at admission: a seeded request (or one that carries
    a `generator`) from its own generator in chunk order -- the generator moves only when the whole request was planned -- and an unseeded
    one from the global generator, in admission order.  `max_frames` caps the summed rows (`dur`) of the units in flight; a request that
    does not fit waits for a later boundary and nothing behind it overtakes it (a request larger than the cap runs when nothing else
    is in flight).  `max_requests` caps the requests in flight the same way.  `span_units` has one entry per span: the units it advanced.
    Every boundary pays one sequence set-up, one text / conditioning / time precompute and the packed state copies again, so a short span
    buys its low admission wait with device time.  `span_steps` defaults to 8: measured on an MI355X (`tools/admission_bench.py`,
    profiles/r07_admission_bench.txt) that boundary cost is 3.3 ms with 8 units in flight, 2.3 % of an 8-step span (4.6 % of a 4-step one),
    and 8 is the shortest span whose median time to result on the trace was not above `MicroBatcher`'s.

    Finished requests leave through `finish_requests`' path with their planned `WaveSpec`; with `device_backend=True` their chunk
    waves stay on the device and their results are int16 PCM from one `ops.wave_finish` call per boundary."""

    def __init__(self, model_obj, vocoder, span_steps=span_steps, max_frames=None, max_requests=None, mel_spec_type=mel_spec_type, target_rms=target_rms,
                 cross_fade_duration=cross_fade_duration, nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef,
                 speed=speed, fix_duration=fix_duration, device=None, tokenizer=text_to_tokens, device_backend=False):
        if not getattr(model_obj, "resumable_spans", False):
            raise ValueError("SpanScheduler needs a model object with resumable spans (plan_unit / advance: F5HipModel)")
        if int(span_steps) < 1:
            raise ValueError(f"span_steps must be at least 1 (got {span_steps})")
        self.model_obj, self.vocoder, self.span_steps = model_obj, vocoder, int(span_steps)
        self.max_frames, self.max_requests = max_frames, max_requests
        self.mel_spec_type, self.target_rms, self.cross_fade_duration = mel_spec_type, target_rms, cross_fade_duration
        self.defaults = dict(speed=speed, nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=None)
        self.fix_duration, self.device, self.tokenizer = fix_duration, device, tokenizer
        self.device_backend = bool(device_backend)   # finished requests leave as int16 PCM, joined and quantised on the device (`finish_requests`)
        self.waiting: list[SpanTicket] = []
        self.in_flight: list[SpanTicket] = []
        self.span_units: list[int] = []

    @property
    def busy(self) -> bool:
        return bool(self.waiting or self.in_flight)

    def prepare(self, requests):
        """The device front-end of the deferred voices (`PreparedVoice.deferred`: uploaded clips) among `requests`, in ONE `prepare_voices`
        call, ahead of their `admit`; a voice that is still deferred at `admit` is prepared there, alone."""
        _prepare_deferred([v for r in requests for v in request_voices(r) if isinstance(v, PreparedVoice)], self.model_obj)

    def admit(self, request) -> SpanTicket:
        plan = plan_request(request, self.defaults, target_rms=self.target_rms, fix_duration=self.fix_duration, device=self.device,
                            tokenizer=self.tokenizer)
        opts = plan.opts
        _prepare_deferred([voice for voice, _ in plan.parts], self.model_obj)   # (a script's uploads that are still deferred: one call)
        extra = {} if opts.get("ode_method") is None else dict(ode_method=opts["ode_method"])   # (handed on only when the request sets it)
        parts = []
        for voice, units in plan.parts:   # segment after segment: the noise is drawn in the script's flat chunk order
            cond = voice.cond(self.model_obj)
            parts.append((voice, [self.model_obj.plan_unit(cond, tokens, frames, steps=int(opts["nfe_step"]), cfg_strength=opts["cfg_strength"],
                                                           sway_sampling_coef=opts["sway_sampling_coef"], generator=plan.generator, **extra)
                                  for tokens, frames in units]))
        plan.commit()   # every chunk was planned: the caller's generator moves
        ticket = SpanTicket(request, plan.voice, [u for _, us in parts for u in us], plan.spec, parts, plan.script)
        self.waiting.append(ticket)
        return ticket

    def _fits(self, ticket) -> bool:
        if not self.in_flight:
            return True
        if self.max_requests is not None and len(self.in_flight) >= self.max_requests:
            return False
        return self.max_frames is None or sum(t.frames for t in self.in_flight) + ticket.frames <= self.max_frames

    def _board(self):
        """A span boundary: cancelled tickets leave, waiting ones join in order of arrival while they fit."""
        self.in_flight = [t for t in self.in_flight if not t.cancelled]
        self.waiting = [t for t in self.waiting if not t.cancelled]
        while self.waiting and self._fits(self.waiting[0]):
            ticket = self.waiting.pop(0)
            ticket.in_flight = True
            self.in_flight.append(ticket)

    def _finish(self, tickets):
        groups = [([u.mel for u in units], voice.ref_frames, voice.rms) for t in tickets for voice, units in t.parts]   # one per segment
        got = _chunk_waves(groups, self.vocoder, self.mel_spec_type, self.target_rms, on_device=self.device_backend, want_specs=False)
        first = np.cumsum([0] + [len(t.parts) for t in tickets])
        chunk_waves = [request_chunk_waves(t, got[first[i]:first[i + 1]]) for i, t in enumerate(tickets)]
        results = _finish_specs(chunk_waves, [request_text(t.request) for t in tickets], self.cross_fade_duration, [t.spec for t in tickets],
                                self.device_backend, "pcm16" if self.device_backend else "float")
        for t, result in zip(tickets, results):
            t.result, t.done, t.in_flight = result, True, False

    def step(self) -> list:
        """One boundary and one span.  Returns the tickets that finished, `result` set."""
        self._board()
        units = [u for t in self.in_flight for u in t.units if not u.done]
        if not units:
            return []
        self.span_units.append(len(units))
        self.model_obj.advance(units, self.span_steps)
        finished = [t for t in self.in_flight if all(u.done for u in t.units)]
        if finished:
            self._finish(finished)   # (a ticket leaves `in_flight` only with its result: a failing vocoder call leaves it to `take_in_flight`)
            self.in_flight = [t for t in self.in_flight if not t.done]
        return finished

    def take_in_flight(self) -> list:
        """Removes and returns every ticket in flight (after a span that raised: the caller retries them with `run_alone`)."""
        taken, self.in_flight = self.in_flight, []
        for t in taken:
            t.in_flight = False
        return taken

    def run_alone(self, ticket, lock=None) -> SpanTicket:
        """The ticket's request on its own, from its first step, with the noise it drew at admission: its units are reset and advanced span
        by span with nothing else in the call, then vocoded.  `lock` (a context manager, e.g. the device lock) is taken for each span and for
        the vocoder call, not for the whole request, so whatever else waits for it waits for one span here too."""
        lock = lock if lock is not None else contextlib.nullcontext()
        for u in ticket.units:
            u.reset()
        while not all(u.done for u in ticket.units):
            with lock:
                self.model_obj.advance([u for u in ticket.units if not u.done], self.span_steps)
        with lock:
            self._finish([ticket])
        return ticket


_VOICE_TAG = re.compile(r"\[(\w+)\]")


def split_voice_tags(text_gen, voices):
    """Multi-voice script -> [(voice, text)] (F/infer/infer_cli.py:181-197): the text is cut in front of every `[tag]`; a piece without a
    tag, or with a tag that is not in `voices`, is spoken by "main"; empty pieces are dropped; the tag itself is not spoken."""
    pieces = []
    for piece in re.split(r"(?=\[\w+\])", text_gen):
        if not piece.strip():
            continue
        m = _VOICE_TAG.match(piece)
        voice = m.group(1) if m and m.group(1) in voices else "main"
        text = _VOICE_TAG.sub("", piece).strip()
        if text:   # (a tag with nothing behind it would hand the reference an empty gen_text; dropped here)
            pieces.append((voice, text))
    return pieces


def infer_multi_voice(text_gen, voices, model_obj, vocoder, **kw):
    """The multi-voice loop of the reference's CLI (F/infer/infer_cli.py:181-208): `voices` = {"main": {"ref_audio": path | (wave, sr),
    "ref_text": str}, "<tag>": {...}}; every `[tag]` piece is synthesized with its voice and the pieces are concatenated (no
    cross-fade between voices, like the reference).  All pieces go to the GPU as ONE `infer_requests` batch instead of one
    `infer_process` call after the other.  Returns (wave, sample_rate, [spectrogram per piece])."""
    if "main" not in voices:
        raise ValueError('voices needs a "main" entry')
    pieces = split_voice_tags(text_gen, voices)
    if not pieces:
        raise ValueError("nothing to synthesize")
    res = infer_requests([(voices[v]["ref_audio"], voices[v]["ref_text"], t) for v, t in pieces], model_obj, vocoder, **kw)
    return np.concatenate([w for w, _, _ in res]), target_sample_rate, [s for _, _, s in res]


# ----------------------------------------- F/infer/speech_edit.py:119-192
max_duration = 4096   # CFM.sample's default clamp (F/model/cfm.py:92,137)


@dataclass(frozen=True)
class EditPlan:
    """What `plan_edit` derives from a recording's length and the spans to regenerate, at hop resolution.
    `segments`: the conditioning wave as ((start, stop, zeros), ...) -- samples [start, stop) of the prepared recording followed by
    `zeros` zero samples; `length`: its length L; `duration`: the frames requested from the sampler (L // 256); `edit_mask`: bool
    [L // 256 + 1], True = keep the frame, False = regenerate it."""
    segments: tuple
    length: int
    duration: int
    edit_mask: torch.Tensor

    def cond(self, audio):
        """The conditioning wave [1, L] built from the prepared recording `audio` [1, n_samples]."""
        parts = []
        for start, stop, zeros in self.segments:
            parts.append(audio[:, start:stop])
            if zeros:
                parts.append(torch.zeros(audio.shape[0], zeros, dtype=audio.dtype, device=audio.device))
        return torch.cat(parts, dim=-1)


def plan_edit(n_samples, parts_to_edit, fix_duration=None, mel_spec_type=mel_spec_type):
    """The splice and mask arithmetic of F/infer/speech_edit.py:129-148 for a recording of `n_samples` samples at 24 kHz (after the
    mono mix and the rms gain); `parts_to_edit` = [[start_s, end_s], ...] on that timeline, `fix_duration` = one length in seconds per
    part or None.  Same rounding as the reference (Python's round: round(112.5) == 112) and the same truncation (the mask is padded with
    True to L // 256 + 1, or cut there, as F.pad does with a negative pad).  `fix_duration` is not mutated (the reference pops it).

    One deliberate difference: the reference builds the spliced wave but never uses it (the line that appends the tail and swaps it
    in is commented out, speech_edit.py:147), so its `cond` is the original recording while a `fix_duration` mask is laid out on the
    spliced timeline -- from the second part on that mask marks the wrong frames.  Here, with `fix_duration=None` the reference is
    reproduced exactly (cond = the recording, L = n_samples); with `fix_duration` the splice that commented line describes is used (the
    kept slices with each part replaced by zeros of its new length, then the tail), so every new span gets its requested length.

    Rejected with ValueError before anything is sized by them: parts that are non-finite, empty, unsorted, overlapping or outside the
    recording; a `fix_duration` of the wrong length or with non-finite or non-positive entries; and an edit whose final frame count
    (the mel frames of `mel_spec_type`'s front-end + 1, cfm.py:136) exceeds the sampler's max_duration, which would clamp the output
    below the mask.  The length and frame count are worked out from the segments first; the mask is built only for an edit that fits."""
    sr = target_sample_rate
    if mel_spec_type not in ("vocos", "bigvgan"):
        raise ValueError(mel_spec_type)
    parts = [list(p) for p in parts_to_edit]
    if not parts:
        raise ValueError("parts_to_edit is empty: give at least one [start, end] span in seconds")
    spans, prev_end = [], 0.0
    for i, p in enumerate(parts):
        if len(p) != 2:
            raise ValueError(f"parts_to_edit[{i}] = {p!r}: expected [start, end] in seconds")
        start, end = float(p[0]), float(p[1])
        if not (math.isfinite(start) and math.isfinite(end)):
            raise ValueError(f"parts_to_edit[{i}] = {p!r}: start and end must be finite numbers of seconds")
        if not end > start:
            raise ValueError(f"parts_to_edit[{i}] = {p!r} is empty: end must be after start")
        if start < 0 or round(end * sr) > n_samples:
            raise ValueError(f"parts_to_edit[{i}] = {p!r} lies outside the recording (0 to {n_samples / sr:.4f} s)")
        if start < prev_end:
            raise ValueError(f"parts_to_edit[{i}] = {p!r} is unsorted or overlaps the previous part (which ends at {prev_end} s)")
        spans.append((start, end))
        prev_end = end
    # the longest edit the sampler can hold: its final frame count (mel frames + 1, cfm.py:136) within max_duration
    max_samples = (max_duration - 1 - _mel_frames(0, mel_spec_type)) * hop_length + hop_length - 1
    if fix_duration is not None:
        fix = [float(d) for d in fix_duration]
        if len(fix) != len(spans):
            raise ValueError(f"fix_duration has {len(fix)} entries for {len(spans)} parts_to_edit")
        if any(not (math.isfinite(d) and d > 0) for d in fix):
            raise ValueError(f"fix_duration = {list(fix_duration)!r}: every entry must be a finite, positive number of seconds")
        if any(d * sr > max_samples for d in fix):   # (bounds every product below before anything is sized by it)
            raise ValueError(f"fix_duration = {list(fix_duration)!r}: an edit longer than {max_samples / sr:.2f} s exceeds the sampler's "
                             f"max_duration of {max_duration} frames")
    # the conditioning wave's segments and length, worked out before the mask is built
    offset = 0
    segments, runs = [], []
    for i, (start, end) in enumerate(spans):
        part_dur = end - start if fix_duration is None else fix[i]
        part_dur = part_dur * sr
        start = start * sr
        segments.append((round(offset), round(start), round(part_dur)))
        runs.append((round((start - offset) / hop_length), round(part_dur / hop_length)))
        offset = end * sr
    if fix_duration is None:
        segments = [(0, n_samples, 0)]
    else:
        segments.append((round(offset), n_samples, 0))
    length = sum(stop - start + zeros for start, stop, zeros in segments)
    if length > max_samples:
        raise ValueError(f"the edited recording needs {_mel_frames(length, mel_spec_type) + 1} frames; the sampler's max_duration is "
                         f"{max_duration} ({max_samples / sr:.2f} s)")
    frames = length // hop_length + 1
    mask = torch.ones(frames, dtype=torch.bool)          # padded with True to L // 256 + 1, or cut there (F.pad, speech_edit.py:148)
    k = 0
    for ones, zeros in runs:
        k += ones
        mask[min(k, frames):min(k + zeros, frames)] = False
        k += zeros
    return EditPlan(tuple(segments), length, length // hop_length, mask)


def _mel_frames(n_samples, mel_spec_type):
    """Frames of the mel front-end of `mel_spec_type` for a wave of n_samples: 1 + n // hop (vocos, centred STFT) or n // hop (bigvgan)."""
    return n_samples // hop_length + (1 if mel_spec_type == "vocos" else 0)


@dataclass(frozen=True)
class PreparedEdit:
    """The host part of one speech edit (`prepare_edit`): the conditioning wave [1, L], the target text's tokens, the plan, the mask cut to
    the mel front-end's frames, the recording's measured rms, and the settings they were made with.  `speech_edit_batch` accepts it
    wherever an (audio, target_text, parts_to_edit, fix_duration) tuple is expected."""
    cond: torch.Tensor
    tokens: list
    plan: EditPlan
    edit_mask: torch.Tensor
    rms: torch.Tensor
    mel_spec_type: str
    target_rms: float


def prepare_edit(audio, target_text, parts_to_edit, fix_duration=None, mel_spec_type=mel_spec_type, target_rms=target_rms, device=None,
                 tokenizer=text_to_tokens):
    """Host part of F/infer/speech_edit.py:120-163 for one edit, no device work: read the recording (a path, WAV bytes or a (tensor, sr)
    pair), mono mix, rms gain to `target_rms` when below it, resample to 24 kHz, `plan_edit`, tokenise, build the conditioning wave.
    Raises ValueError for an empty text, a text with more tokens than the recording has mel frames, or a rejected plan."""
    if not isinstance(target_text, str) or not target_text.strip():
        raise ValueError("target_text is empty: give the full transcript of the edited recording")
    wav, sr = audio if isinstance(audio, tuple) else load_audio(audio)
    wav, rms = _prepare_reference(wav, sr, target_rms, None)
    plan = plan_edit(wav.shape[-1], parts_to_edit, fix_duration, mel_spec_type)
    tokens = tokenizer([target_text])[0]
    frames = _mel_frames(plan.length, mel_spec_type)
    if len(tokens) > frames:
        raise ValueError(f"target_text has {len(tokens)} tokens, more than the {frames} mel frames of the "
                         f"{plan.length / target_sample_rate:.2f} s recording")
    cond = plan.cond(wav)
    return PreparedEdit(cond if device is None else cond.to(device), tokens, plan, plan.edit_mask[:frames], rms, mel_spec_type, target_rms)


def speech_edit_batch(edits, model_obj, vocoder, mel_spec_type=mel_spec_type, target_rms=target_rms, nfe_step=nfe_step,
                      cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=None, device=None, tokenizer=text_to_tokens,
                      generators=None, ode_method=None):
    """Several speech edits in ONE sampler call: `edits` = [(audio, target_text, parts_to_edit, fix_duration) | PreparedEdit], `audio` a
    path, the bytes of a WAV file, or a (tensor, sr) pair.  Returns one (wave float32, 24000, spec [100, T]) triple per edit, each what
    `speech_edit` returns for that edit alone: every edit keeps the reference's batch-1 semantics (its own prompt length `lens` and its
    own edit mask), its noise is drawn in order like sequential calls draw it, and it is vocoded and rms-restored on its own.  Bit for
    bit this holds when the model handle runs the shape-invariant attention arithmetic (see `infer_requests`).

    Per edit, F/infer/speech_edit.py:120-192: `prepare_edit` (mono mix, rms gain, 24 kHz, `plan_edit`, tokens); `sample(cond, text,
    duration=L // 256, edit_mask)`; vocode every frame (`ref_audio_len = 0`); restore the rms.  Text goes through `text_to_tokens`, the
    tokenisation `infer_process` uses (the script's non-pinyin branch wraps the list once more, `[text_list]`).
    With mel_spec_type="bigvgan" the front-end yields L // 256 mel frames, one fewer than the reference's mask, which then fails to
    broadcast in `cond_mask & edit_mask` (cfm.py:130); the mask is cut to the mel's frames here, its last entry having no frame.

    The model object needs the reference's `sample()`; with `cond_mel` (F5HipModel) the edits are handed over as one padded mel batch,
    any other object is driven edit by edit with the raw wave, like the reference does.  `generators` ([torch.Generator | None] per edit,
    `request_generator`): an edit's noise comes from its own generator instead of the global one (F5HipModel only).  `ode_method`: one
    solver name for the call or one name (or None) per edit, handed to `sample()` only when an edit names one."""
    if mel_spec_type not in ("vocos", "bigvgan"):
        raise ValueError(mel_spec_type)
    preps = []
    for e in edits:
        if isinstance(e, PreparedEdit):
            if (e.mel_spec_type, e.target_rms) != (mel_spec_type, target_rms):
                raise ValueError(f"PreparedEdit made for mel_spec_type={e.mel_spec_type!r}, target_rms={e.target_rms}; this call uses "
                                 f"{mel_spec_type!r}, {target_rms}")
            preps.append(e if device is None else dataclasses.replace(e, cond=e.cond.to(device)))
        else:
            audio, target_text, parts_to_edit, fix_duration = e
            preps.append(prepare_edit(audio, target_text, parts_to_edit, fix_duration, mel_spec_type, target_rms, device, tokenizer))
    knobs = dict(steps=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed)
    methods = list(ode_method) if isinstance(ode_method, (list, tuple)) else [ode_method] * len(preps)
    if len(methods) != len(preps):
        raise ValueError(f"ode_method: one name per edit ({len(preps)}) or one name, got {len(methods)}")
    if generators is not None and any(g is not None for g in generators):
        if not hasattr(model_obj, "cond_mel") or len(generators) != len(preps):
            raise ValueError("generators: one per edit, and a model object with cond_mel (F5HipModel)")
        knobs["generators"] = list(generators)
    if hasattr(model_obj, "cond_mel"):
        mels = [model_obj.cond_mel(p.cond)[0] for p in preps]
        lens = torch.tensor([m.shape[0] for m in mels], dtype=torch.long)
        edit_mask = torch.zeros(len(preps), int(lens.max()), dtype=torch.bool)    # (past an edit's lens its cond_mask is False anyway)
        for i, p in enumerate(preps):
            edit_mask[i, :p.edit_mask.shape[0]] = p.edit_mask
        out, _ = model_obj.sample(cond=torch.nn.utils.rnn.pad_sequence(mels, batch_first=True), text=[p.tokens for p in preps],
                                  duration=torch.tensor([p.plan.duration for p in preps], dtype=torch.long), lens=lens,
                                  edit_mask=edit_mask, **knobs, **(dict(ode_method=ode_method) if any(m is not None for m in methods) else {}))
        # each edit's rows: its final duration max(lens + 1, L // 256) (cfm.py:136), i.e. lens + 1
        gens = [out[i, :max(int(lens[i]) + 1, p.plan.duration)] for i, p in enumerate(preps)]
    else:
        gens = [model_obj.sample(cond=p.cond, text=[p.tokens], duration=p.plan.duration, edit_mask=p.edit_mask[None], **knobs,
                                 **({} if name is None else dict(ode_method=name)))[0][0] for p, name in zip(preps, methods)]
    res = []
    for gen, p in zip(gens, preps):
        wave, sr, spec = _vocode_and_join([gen], 0, p.rms, vocoder, mel_spec_type, target_rms, 0)
        res.append((np.asarray(wave, dtype=np.float32), sr, spec))
    return res


def speech_edit(audio, target_text, parts_to_edit, model_obj, vocoder, fix_duration=None, mel_spec_type=mel_spec_type,
                target_rms=target_rms, nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef,
                seed=None, device=None, ode_method=None):
    """F/infer/speech_edit.py:119-192 as a call: regenerate `parts_to_edit` ([[start_s, end_s], ...]) of the recording `audio` (a path,
    WAV bytes or a (tensor, sr) pair) so that it speaks `target_text` (the full new transcript) in the same voice, keeping every other
    frame.  Returns (wave float32, 24000, spec [100, T]).  `speech_edit_batch` with one edit; see there and `plan_edit`."""
    return speech_edit_batch([(audio, target_text, parts_to_edit, fix_duration)], model_obj, vocoder, mel_spec_type=mel_spec_type,
                             target_rms=target_rms, nfe_step=nfe_step, cfg_strength=cfg_strength,
                             sway_sampling_coef=sway_sampling_coef, seed=seed, device=device, ode_method=ode_method)[0]
