"""`/v1/audio/speech` over the HIP path: the reference's route, request model, manager and helper with
the same names, status codes and response shape, and a local voice registry instead of a GitHub fetch per request.

Mirrors: `S/routes/speech.py:19-41` (route), `S/utils/tts_utils.py:22-65` (`KannadaSynthesizeRequest`,
`SynthesizeRequest`, `synthesize_speech`), `S/core/managers.py:62-85` (`TTSManager`: `.model`, `.load()`,
`.synthesize(text, ref_audio_path, ref_text)`).  Only this path of the server is built: no auth, rate limiting, logging
configuration, ASR / LLM / translation routes (out of scope).

Differences, explicit:
  * reference voices come from `VoiceRegistry` (name -> local 16-bit WAV + transcript); the reference downloads the prompt WAV
    from GitHub on every request (`tts_utils.py:40-46`), which this deployment target (no egress) cannot and should not do;
  * the response body is 16-bit PCM WAV at 24 kHz written with the stdlib (`soundfile`'s default WAV subtype for float input
    is PCM_16 as well); the bytes of a body -- `wav_bytes`, `wav_stream_header`, `delivery_bytes`, `pcm16` -- are made in the leaf module
    `wave_codec`, next to the delivery formats they write, and handed on here under the same names;
  * `TTSManager.load()` takes the model / vocoder objects (or a loader callable): checkpoints are not fetched from the hub;
  * `TTSManager(micro_batch=dict(max_requests=16, max_wait_ms=5))`: concurrent requests are collected for a few milliseconds and synthesized as ONE
    sampler batch (`infer.infer_requests`); with `ShardedSampler` as the model object that batch is dealt over the GPUs of the node
    (rank 0 serves HTTP and owns the queue, the other ranks sit in `rank_worker_loop`).  The reference serves one request at a
    time on one GPU (`S/routes/speech.py:19-41`).  A request's result does not depend on its batch: `load()` puts the model handle into
    the library's shape-invariant attention mode (`batch_invariant=True`); without it the same utterance alone and inside a batch can take
    different attention kernels, which agree to the last bits per launch but -- in the mixed GEMM mode -- drift apart to that mode's
    rounding-noise floor over a sample (measured 4.4e-4 rms after two Euler steps, `profiles/r03_attn_mode_tapdiff.txt`).
  * `POST /v1/audio/edit` + `TTSManager.edit`: the reference's speech-edit script (F/infer/speech_edit.py, a CLI there) as a route; the
    recording arrives base64-encoded in a JSON body (multipart uploads need python-multipart, which this image does not have).
"""

import base64
import binascii
import collections
import hashlib
import io
import logging
import queue
import threading
import time
import types
import typing
from concurrent.futures import Future
from dataclasses import dataclass, field
from typing import Callable

import math

import numpy as np

from . import audio_prep, infer
from .wave_codec import delivery_bytes, pcm16, wav_bytes, wav_stream_header  # noqa: F401  (handed on: serve.wav_bytes, serve.pcm16, ...)

log = logging.getLogger(__name__)

EDIT_OPTIONS = ("nfe_step", "cfg_strength", "sway_sampling_coef", "seed", "ode_method", "flac_level")   # a speech edit has no `speed`: its durations are planned
# the delivery options an edit takes, in the order the routes check them (`infer.REQUEST_OPTIONS`'): all but `remove_silence`, the recording keeps its pauses
EDIT_DELIVERY = tuple(k for k in infer.REQUEST_OPTIONS if k in infer.DELIVERY_OPTIONS and k != "remove_silence")
EDIT_MARK = infer.WATERMARK_OPTIONS   # and the mark, in the same `infer.WaveSpec`: the whole returned recording is marked (`infer.mark_pcm16`), on the host, as the route finishes
# most ODE steps one library call accepts per method: 128 time points (f5hip precompute_time); midpoint uses 2 per step, RK4 3 per step + 1
MAX_NFE_STEP = {"euler": 128, "midpoint": 64, "rk4": 42}


def check_request_options(options: dict, ode_method: str = "euler", allowed=infer.REQUEST_OPTIONS, watermark=None) -> dict:
    """The per-request sampler options a client set (None = not set, dropped), checked before anything is queued: ValueError with a message
    the routes return as 400.  `speed` finite and > 0; `nfe_step` an integer in 1..MAX_NFE_STEP[ode_method]; `cfg_strength` and
    `sway_sampling_coef` finite; `seed` an integer in 0..2**63 - 1; `ode_method` one of MAX_NFE_STEP's names.  `ode_method` (the argument)
    is the model's solver: `nfe_step`'s upper limit follows the request's own `ode_method` when it sets one, else the model's.
    The delivery options by `infer.WaveSpec`'s validators, one by one and then together (a `flac_level` beside another encoding is refused,
    never ignored; a `tempo` and a `pitch` whose combined stretch leaves 1/2 .. 2 likewise); `remove_silence` must be a bool, and `flac_level`
    is not "1".  What a request gets anyway -- False, 24000, "pcm16", level 0, tempo 1.0, pitch 0 -- is dropped like None: the request is
    then what it is without the option.  `watermark` by `infer.check_watermark`: an integer key from 1 to 2^48 - 1, or `{"key": K, "id": I}`
    with a trace id from 0 to 2^30 - 1 (an `infer.WatermarkTag`); `{"id": I}` alone takes the key of `watermark` (the argument: the
    service's own key or tag) and is refused without one.  `keep_formants` by
    `infer.check_keep_formants`: a bool (false is dropped), and true only beside a non-zero `pitch`."""
    out = {}
    own = options.get("ode_method") if "ode_method" in allowed else None
    if own is not None:
        if not isinstance(own, str) or own not in MAX_NFE_STEP:
            raise ValueError(f"ode_method must be one of 'euler', 'midpoint', 'rk4' (got {own!r})")
        ode_method = own
    for k, v in options.items():
        if k not in allowed:
            raise ValueError(f"unknown option {k!r} (allowed: {', '.join(allowed)})")
        if v is None:
            continue
        if k == "ode_method":
            pass
        elif k == "remove_silence":
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"remove_silence must be true or false (got {v!r})")
            if not v:
                continue
            v = True
        elif k in ("sample_rate", "encoding"):
            i = ("sample_rate", "encoding").index(k)
            v = infer.delivery_format(**{k: v})[i]      # ValueError: "<name> must be one of ..."
            if v == infer.delivery_format()[i]:         # 24000 / "pcm16": what a request gets anyway
                continue
        elif k == "loudness":
            v = infer.check_loudness(v)                 # ValueError: "loudness must be ..."
        elif k == "flac_level":
            v = infer.check_flac_level(v)               # ValueError: "flac_level must be one of ..."
        elif k == "tempo":
            v = infer.check_tempo(v) / 100              # ValueError: "tempo must be a number from 0.5 to 2 ..."
            if v == 1.0:
                continue
        elif k == "pitch":
            v = infer.check_pitch(v)                    # ValueError: "pitch must be a whole number of semitones ..."
            if v == 0:
                continue
        elif k == "watermark":
            v = infer.check_watermark(v, watermark)     # ValueError: "watermark must be an integer key ...", "watermark id must be ..."
        elif k == "keep_formants":
            if not infer.check_keep_formants(v):        # ValueError: "keep_formants must be true or false ..."
                continue
            v = True
        elif k in ("nfe_step", "seed"):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{k} must be an integer (got {v!r})")
            v = int(v)
            if k == "nfe_step":
                hi = MAX_NFE_STEP[ode_method]
                if not 1 <= v <= hi:
                    raise ValueError(f"nfe_step must be between 1 and {hi} for the {ode_method} solver (got {v}).")
            elif not 0 <= v < 2 ** 63:
                raise ValueError(f"seed must be between 0 and 2**63 - 1 (got {v}).")
        else:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"{k} must be a number (got {v!r})")
            v = float(v)
            if not math.isfinite(v):
                raise ValueError(f"{k} must be a finite number (got {v}).")
            if k == "speed" and v <= 0:
                raise ValueError(f"speed must be greater than 0 (got {v}).")
        out[k] = v
    infer.WaveSpec.of(out)                              # the wave options together.  ValueError: "flac_level needs encoding 'flac' ...", then "keep_formants needs a non-zero pitch"
    if out.get("flac_level") == 0:
        del out["flac_level"]
    return out


# Whether uploaded reference clips take the device front-end unless `TTSManager(device_frontend=...)` says otherwise: it does when it beat
# the host front-end for ONE clip by more than that run's own spread (tools/ref_frontend_bench.py, profiles/ref_frontend_bench.txt)
DEVICE_FRONTEND_DEFAULT = True
# Whether finished waves are joined, quantised and stripped of pauses on the device unless `TTSManager(device_backend=...)` says otherwise.
# Off: turning it on changes what `synthesize` returns (int16 PCM instead of float32), and the rule above asks for a win at ONE request by
# more than the run's own spread (tools/wave_backend_bench.py, profiles/wave_backend_bench.txt; DESIGN "Waveform back-end")
DEVICE_BACKEND_DEFAULT = False
# Whether FLAC uploads and recordings are decoded on the device (`ops.flac_decode`) unless `TTSManager(device_decode=...)` says otherwise: it
# is on because the device beat the host's `read_flac` for ONE clip on the MI355X -- 10 s stereo 44.1 kHz, block 4096, LPC order 8: host
# 1426.2 ms (1423.3 .. 1434.7), device 13.7 ms (13.6 .. 13.9), upload, download and MD5 included (tools/flac_decode_bench.py,
# profiles/flac_decode_bench.txt).  The samples are the same either way.
DEVICE_DECODE_DEFAULT = True
# Whether an uploaded clip's silence pre-step (clip at a pause, strip the edges, 50 ms tail) runs on the device (`ops.ref_prestep`) unless
# `TTSManager(device_prestep=...)` says otherwise.  Off: the option is new, and its measurement (tools/ref_prestep_bench.py,
# profiles/ref_prestep_bench.txt) decides nothing about the default.  The samples are the same either way.
DEVICE_PRESTEP_DEFAULT = False
STREAM_REMOVE_SILENCE = "remove_silence needs the request's whole wave: it is not available on a streaming path"
STREAM_LOUDNESS = "loudness is measured on the request's whole wave: it is not available on a streaming path"
STREAM_PROSODY = "tempo and pitch are applied to the request's whole wave: they are not available on a streaming path"
STREAM_WATERMARK = "watermark marks the request's whole wave: it is not available on a streaming path"
MARKED_REFERENCE = infer.MARKED_REFERENCE   # "the reference clip carries this service's watermark": `TTSManager(reject_marked=...)`


def stream_refusal(opts):
    """The message a streaming path refuses `opts` with, or None: an option that needs the whole wave (`infer.needs_whole_wave`; the
    delivery format does not count, a stream applies it piece by piece)."""
    spec = infer.WaveSpec.of(opts)
    if not spec.needs_whole_wave(streamed=True):
        return None
    if spec.remove_silence:
        return STREAM_REMOVE_SILENCE
    if spec.loudness is not None:
        return STREAM_LOUDNESS
    return STREAM_PROSODY if spec.prosody else STREAM_WATERMARK


@dataclass
class Voice:
    audio_path: str
    ref_text: str


@dataclass
class VoiceRegistry:
    """Local replacement of the reference's EXAMPLES table (`S/utils/tts_utils.py:12-19`): audio_name -> prompt clip + transcript."""
    voices: dict = field(default_factory=dict)
    default_voice: str = "KAN_F (Happy)"

    def add(self, name: str, audio_path: str, ref_text: str) -> None:
        self.voices[name] = Voice(audio_path, ref_text)

    def get(self, name: str):
        return self.voices.get(name)


class _QueueWorker:
    """What the two batchers share: the queue of (request, future, on_start) items, one worker thread running the subclass's `_loop`,
    and the shutdown protocol -- `close()` puts a mark (None) behind everything that was accepted, refuses later submits, waits for the
    worker and fails whatever it left behind with RuntimeError("<class name> is closed").  A subclass sets what its loop needs before it
    calls `__init__` here, which starts the thread."""

    def __init__(self, thread_name: str):
        self._q: queue.Queue = queue.Queue()
        self._closed = False
        self._gate = threading.Lock()             # orders submit() against close(): no item can land behind the shutdown mark
        self._thread = threading.Thread(target=self._loop, name=thread_name, daemon=True)
        self._thread.start()

    def _closed_error(self):
        return RuntimeError(f"{type(self).__name__} is closed")

    def submit(self, request, on_start: Callable[[], None] | None = None) -> Future:
        f: Future = Future()
        with self._gate:
            if self._closed:
                raise self._closed_error()
            self._q.put((request, f, on_start))
        return f

    def close(self, timeout: float = 30.0):
        with self._gate:
            if self._closed:
                return
            self._closed = True
            self._q.put(None)                     # the shutdown mark: everything in front of it is still served
        self._thread.join(timeout=timeout)
        self._fail_pending()                      # (only non-empty if the worker thread did not get there: join timed out)

    def _fail_pending(self):
        while True:
            try:
                item = self._q.get_nowait()
            except queue.Empty:
                return
            if item is not None and item[1].set_running_or_notify_cancel():
                item[1].set_exception(self._closed_error())


class MicroBatcher(_QueueWorker):
    """Collects concurrent synthesis requests into one sampler batch.

    `submit((ref_audio, ref_text, gen_text))` returns a `concurrent.futures.Future`; a single worker thread takes the first waiting
    request, keeps collecting for at most `max_wait_ms` or until `max_requests` are waiting, runs `run_batch(list_of_requests)` (one
    `infer.infer_requests` call = one library call over all chunks of all requests) and resolves the futures in order.  One batch is in
    flight at a time -- the library allows one call per handle -- and the next one forms while it runs, so under load the batch size
    grows by itself.  A failing batch is retried request by request so one bad request cannot fail its neighbours -- unless the error
    says the backend itself is gone (`no_retry`, e.g. a rank of a sharded job failed): then the whole batch fails at once.
    `close()` resolves every request that is still queued with RuntimeError("MicroBatcher is closed"); nothing can be enqueued behind it.
    A request whose future was cancelled while it waited (a streaming client that went away) is dropped when its batch forms, before
    `run_batch`; `submit(request, on_start=fn)` calls `fn()` on the worker thread once the request's batch has formed and before it runs,
    so anything submitted from `fn` rides in a later batch (a stream's remaining chunks behind its first chunk)."""

    def __init__(self, run_batch: Callable[[list], list], max_requests: int = 16, max_wait_ms: float = 5.0):
        self.run_batch, self.max_requests, self.max_wait = run_batch, int(max_requests), max_wait_ms / 1e3
        self.batch_sizes: list[int] = []          # observability: sizes of the batches run so far
        super().__init__("f5hip-microbatcher")

    def _collect(self):
        first = self._q.get()
        if first is None:
            return None
        batch, deadline = [first], time.monotonic() + self.max_wait
        while len(batch) < self.max_requests:
            left = deadline - time.monotonic()
            try:
                item = self._q.get(timeout=left) if left > 0 else self._q.get_nowait()
            except queue.Empty:
                break
            if item is None:
                self._q.put(None)   # leave the shutdown mark for the loop (nothing can follow it: submit() is closed)
                break
            batch.append(item)
        return batch

    def _loop(self):
        while True:
            batch = self._collect()
            if batch is None:       # the shutdown mark: every request submitted before close() has been served
                break
            batch = [item for item in batch if item[1].set_running_or_notify_cancel()]   # cancelled while queued: never run
            if not batch:
                continue
            self.batch_sizes.append(len(batch))
            for _, _, on_start in batch:
                if on_start is not None:
                    try:
                        on_start()
                    except Exception:   # noqa: BLE001 -- a hook must not stop the worker; its owner sees the missing follow-up
                        pass
            try:
                results = self.run_batch([item[0] for item in batch])
                if len(results) != len(batch):
                    raise RuntimeError(f"run_batch returned {len(results)} results for {len(batch)} requests")
                for item, res in zip(batch, results):
                    item[1].set_result(res)
            except Exception as e:   # noqa: BLE001 -- isolate the failing request
                if len(batch) == 1 or getattr(e, "no_retry", False):
                    for item in batch:
                        item[1].set_exception(e)
                    continue
                for item in batch:
                    try:
                        item[1].set_result(self.run_batch([item[0]])[0])
                    except Exception as e1:   # noqa: BLE001
                        item[1].set_exception(e1)
        self._fail_pending()


class ContinuousBatcher(_QueueWorker):
    """`MicroBatcher`'s interface over an `infer.SpanScheduler`: requests join the batch that is running at its next span boundary instead of
    waiting for it to end.

    `submit(request, on_start=None)` returns a `concurrent.futures.Future`.  One worker thread alternates between admission and spans: it
    blocks on the queue only while nothing is in flight; otherwise it takes what has arrived without waiting, admits it
    (`scheduler.admit`: the request is planned and draws its noise -- an uploaded clip's front-end runs first, together with those of the
    uploads already queued, `_prepare`; `on_start()` is called right after, so what it submits is admitted at
    the next boundary -- a stream's tail right behind its head), runs ONE span (`scheduler.step()`) under `lock` -- `TTSManager` passes
    its device lock, so a speech edit runs between two spans -- and resolves the futures of the requests that finished.  A request whose
    planning fails gets that error alone.  A future stays cancellable until it is resolved: cancelled while queued it is never admitted,
    cancelled while in flight its units leave at the next boundary.  If a span raises, the requests in flight are retried one at a time
    from their first step with the noise they already drew (`scheduler.run_alone`), so one bad request cannot fail its neighbours -- unless
    the error is marked `no_retry` or only one request was in flight: then they fail at once.  `close()` as `MicroBatcher.close()`:
    everything submitted before it is served, nothing stays unresolved, later submits are refused.  `batch_sizes`: per span, the units
    it advanced."""

    def __init__(self, scheduler, lock=None):
        self.scheduler = scheduler
        self._lock = lock if lock is not None else threading.Lock()
        self._futures: dict = {}                  # ticket -> future, admitted and unresolved (worker thread only)
        super().__init__("f5hip-continuous-batcher")

    @property
    def batch_sizes(self) -> list:
        return self.scheduler.span_units

    @staticmethod
    def _resolve(future, result=None, error=None):
        if future.set_running_or_notify_cancel():     # False: cancelled in the meantime, its waiters are told
            if error is not None:
                future.set_exception(error)
            else:
                future.set_result(result)

    def _prepare(self, request):
        """Ahead of admitting a request whose voice is an upload that is still deferred: its front-end together with that of every deferred
        voice already waiting in the queue, in ONE `scheduler.prepare` call under the lock, so uploads that arrive together share one
        ragged device call and the queued ones find their voice prepared when their turn comes.  Admission itself stays one request at a
        time, in order.  A failure here is logged and left to the admissions: each then prepares its own voice and fails alone."""
        prepare = getattr(self.scheduler, "prepare", None)
        def deferred(r):
            return any(getattr(v, "pending", None) is not None for v in infer.request_voices(r))

        if prepare is None or not deferred(request):
            return
        with self._q.mutex:
            queued = [item[0] for item in self._q.queue if item is not None and not item[1].cancelled()]
        try:
            with self._lock:
                prepare([request] + [r for r in queued if deferred(r)])
        except Exception:   # noqa: BLE001
            log.exception("preparing uploaded reference clips together failed; each request now prepares its own")

    def _admit(self, request, future, on_start):
        if future.cancelled():                        # cancelled while queued: never admitted
            future.set_running_or_notify_cancel()
            return
        self._prepare(request)
        try:
            with self._lock:
                ticket = self.scheduler.admit(request)
        except Exception as e:   # noqa: BLE001 -- a request that cannot be planned fails alone
            self._resolve(future, error=e)
            return
        self._futures[ticket] = future
        if on_start is not None:
            try:
                on_start()
            except Exception:   # noqa: BLE001 -- a hook must not stop the worker; its owner sees the missing follow-up
                pass

    def _span(self):
        for ticket, future in list(self._futures.items()):
            if future.cancelled():                    # cancelled while in flight (or waiting for room): leaves at this boundary
                ticket.cancel()
                future.set_running_or_notify_cancel()
                del self._futures[ticket]
        try:
            with self._lock:
                finished = self.scheduler.step()
        except Exception as e:   # noqa: BLE001 -- isolate the failing request
            failed = self.scheduler.take_in_flight()
            for ticket in failed:
                future = self._futures.pop(ticket)
                if len(failed) == 1 or getattr(e, "no_retry", False):
                    self._resolve(future, error=e)
                    continue
                try:
                    self.scheduler.run_alone(ticket, lock=self._lock)     # the lock per span here too
                    self._resolve(future, ticket.result)
                except Exception as e1:   # noqa: BLE001
                    self._resolve(future, error=e1)
            return
        for ticket in finished:
            self._resolve(self._futures.pop(ticket), ticket.result)

    def _loop(self):
        closing = False
        while not (closing and not self.scheduler.busy):
            block = not self.scheduler.busy           # nothing to advance: wait for a request (or the shutdown mark)
            while not closing:
                try:
                    item = self._q.get() if block else self._q.get_nowait()
                except queue.Empty:
                    break
                block = False
                if item is None:                      # nothing can follow the mark: submit() is closed
                    closing = True
                else:
                    self._admit(*item)
            if self.scheduler.busy:
                self._span()
        self._fail_pending()


class SynthesisStream:
    """Iterator of float32 pieces (`TTSManager.synthesize_stream`).  `close()` may be called from any thread, also while another thread
    waits inside `next()`: it cancels the request's remaining chunks if their batch has not started, and the waiting `next()` then ends
    with `concurrent.futures.CancelledError`."""

    def __init__(self, gen, cancel):
        self._gen, self._cancel = gen, cancel

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._gen)

    def close(self):
        self._cancel()
        try:
            self._gen.close()
        except ValueError:          # the generator is running on another thread: it stops at its wait for the cancelled tail
            pass


class TTSManager:
    """`S/core/managers.py:62-85`.  `model` is what `synthesize` calls: (text, ref_audio_path=..., ref_text=...) -> waveform."""

    def __init__(self, loader: Callable[[], tuple] | None = None, nfe_step: int = infer.nfe_step, cfg_strength: float = infer.cfg_strength,
                 sway_sampling_coef: float = infer.sway_sampling_coef, speed: float = infer.speed, mel_spec_type: str = "vocos",
                 micro_batch: dict | None = None, batch_invariant: bool = True, clip_cache: int = 64, device_frontend: bool | None = None,
                 device_backend: bool | None = None, device_decode: bool | None = None, device_prestep: bool | None = None,
                 watermark=None, reject_marked=None, reference_limits: dict | None = None):
        self.loader = loader
        # The key (`infer.check_watermark`) every finished wave is marked with unless its request names its own; None: no mark.  A mark needs
        # the whole wave, so with a key here the streaming paths are refused (`STREAM_WATERMARK`) rather than left unmarked.  A tag
        # (`{"key": K, "id": I}`, e.g. one id per deployment) marks every such wave with its trace id too; a request's `{"id": I}` takes
        # the key from here.
        self.watermark = infer.check_watermark(watermark)
        # Keys (1 .. 16, or one) whose mark an uploaded reference clip must not carry: a new upload whose prepared 24 kHz wave scores at or
        # above `infer.WATERMARK_THRESHOLD` for any of them is refused (`MARKED_REFERENCE`) before it is denoised, cached or queued.  None: no check
        self.reject_marked = None if reject_marked is None else tuple(infer.check_watermark_keys(reject_marked))
        # The upload gate: any of `infer.REFERENCE_LIMITS` (min_seconds, max_clip_ratio, min_snr_db, min_speech_ratio, min_bandwidth_hz) -> number.
        # A new clone or script upload is measured (`audio_prep.assess_reference`; with `device_frontend` one `ops.ref_assess` call per
        # front-end call) and one that violates a limit is refused with a ValueError naming the measure, its value and the limit -- before the
        # denoiser, the cache and the queue, once per upload.  `min_snr_db` is not applied to a voice with `denoise`.  There are no built-in
        # thresholds: None means no gate, and nothing is measured.  Registered voices are not gated.
        self.reference_limits = infer.check_reference_limits(reference_limits)
        self.batch_invariant = batch_invariant   # False: leave the model's attention mode alone (fastest kernel per launch shape)
        self.micro_batch = micro_batch            # e.g. dict(max_requests=16, max_wait_ms=5): batch concurrent requests; with span_steps
        #                                           (dict(span_steps=8, max_frames=32768); span_steps=None: infer.span_steps) requests join a
        #                                           running batch between spans
        self.batcher: MicroBatcher | ContinuousBatcher | None = None
        self.model = None
        self.model_obj = None
        self.vocoder = None
        self.opts = dict(nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, speed=speed)
        self.mel_spec_type = mel_spec_type
        self._prep_cache: dict = {}   # prompt path -> (PreparedVoice, ref_text): clip / trim / resample / mel run once per voice
        self._prep_lock = threading.Lock()   # route handlers run in a thread pool: concurrent first requests of a voice prepare it once
        # Uploaded clips (`synthesize_clip`): (sha1 of the upload, ref_text, clip_short, denoise) -> (PreparedVoice, ref_text), least recently used
        # first, at most `clip_cache` entries (each holds the prepared wave and its device mel).  `_clip_lock` guards the two tables only;
        # the preparation itself runs under the key's own lock, so one slow upload does not stall other voices.
        self.clip_cache = int(clip_cache)
        self._clip_cache: collections.OrderedDict = collections.OrderedDict()
        self._clip_key_locks: dict = {}      # key -> [lock, threads using it]
        self._clip_lock = threading.Lock()
        # True: an uploaded clip's mono mix / rms gain / resampling run on the device (`infer.prepare_voices`, one ragged call for all new
        # voices of a batch); False: on the host, before the request is queued.  None: DEVICE_FRONTEND_DEFAULT (profiles/ref_frontend_bench.txt)
        self.device_frontend = DEVICE_FRONTEND_DEFAULT if device_frontend is None else bool(device_frontend)
        # True: a batch's chunk waves stay on the device and ONE `ops.wave_finish` call turns them into every request's int16 PCM (cross-fade,
        # quantisation, `remove_silence`), downloaded once; a non-streamed request's result is then that int16 array, which `wav_bytes` passes
        # through -- the same bytes as the float32 wave gives.  False: joined on the host, float32 as before.  None: DEVICE_BACKEND_DEFAULT
        self.device_backend = DEVICE_BACKEND_DEFAULT if device_backend is None else bool(device_backend)
        # True: a FLAC upload or recording is decoded by `ops.flac_decode` (one library call, five launches, under the device lock; with a
        # `ShardedSampler` on rank 0's device); False: by `wave_codec.read_flac` on the host.  None: DEVICE_DECODE_DEFAULT.  WAV never
        # touches the device here.
        self.device_decode = DEVICE_DECODE_DEFAULT if device_decode is None else bool(device_decode)
        # True: an uploaded clip's silence pre-step runs in `ops.ref_prestep` (one library call, three launches, under the device lock) and the
        # clip stays on the device for the front-end; the new uploads of a script share ONE call per distinct rate.  Honoured only with
        # `device_frontend` and a model on a GPU; else `audio_prep.preprocess_ref_segment` on the host.  None: DEVICE_PRESTEP_DEFAULT
        self.device_prestep = DEVICE_PRESTEP_DEFAULT if device_prestep is None else bool(device_prestep)
        # The library allows ONE call in flight per handle (include/f5hip.h), the sampler keeps per-call state and noise comes from torch's
        # global generator: every entry into the device path takes this lock.  Without a batcher, concurrent HTTP requests therefore run one
        # after the other, like the reference's blocking `async def` handlers (S/routes/speech.py:19-41).
        self._device_lock = threading.Lock()
        self.request_timeout_s = 600.0       # a request never waits for its batch for ever

    @property
    def ode_method(self) -> str:
        """The loaded handle's ODE method ("euler" when the model object does not say): bounds a request's `nfe_step`."""
        local = getattr(self.model_obj, "local", self.model_obj)
        return (getattr(local, "odeint_kwargs", None) or {}).get("method", "euler")

    def request_options(self, allowed=infer.REQUEST_OPTIONS, **options) -> dict:
        """`check_request_options` for this manager's solver: the options a request sets (absent / None ones fall back to `self.opts`)."""
        out = check_request_options(options, self.ode_method, allowed, self.watermark)
        if self.watermark is not None and "watermark" in allowed:
            out.setdefault("watermark", self.watermark)   # the manager's key for a request that names none
        return out

    def load(self, model_obj=None, vocoder=None):
        """Attach the sampler / vocoder objects (F5HipModel, F5HipVocos | F5HipBigVGAN), or build them with `loader`."""
        if not self.model:
            if model_obj is None:
                if self.loader is None:
                    raise ValueError("TTSManager.load needs a model object or a loader")
                model_obj, vocoder = self.loader()
            self.model_obj, self.vocoder = model_obj, vocoder
            # A served request must not depend on what it happened to be batched with: this handle runs the shape-invariant attention
            # arithmetic (per-handle setting of the library, ~3 % at batch 1; other handles of the process keep theirs).
            setter = getattr(getattr(model_obj, "local", model_obj), "set_attention_shape_invariant", None)
            if callable(setter) and self.batch_invariant:
                setter(True)
            self.model = self._call
            if self.micro_batch is not None and "span_steps" in self.micro_batch:
                # continuous batching: requests join the running batch at its next span boundary (infer.SpanScheduler)
                if not getattr(model_obj, "resumable_spans", False):
                    self.model = self.model_obj = self.vocoder = None
                    raise ValueError("micro_batch with span_steps needs a model object that samples in resumable spans (F5HipModel); "
                                     f"{type(model_obj).__name__} does not")
                mb = dict(self.micro_batch)
                mb.pop("max_wait_ms", None)      # nothing is waited for: a request joins at the next boundary
                if mb["span_steps"] is None:     # dict(span_steps=None): the scheduler's default
                    del mb["span_steps"]
                sched = infer.SpanScheduler(model_obj, vocoder, mel_spec_type=self.mel_spec_type, device_backend=self.device_backend, **mb, **self.opts)
                self.batcher = ContinuousBatcher(sched, lock=self._device_lock)
            elif self.micro_batch is not None:
                self.batcher = MicroBatcher(self._run_batch, **self.micro_batch)
        return self

    def _run_batch(self, requests):
        """One `infer_requests` call.  A request whose text is a string gets its joined wave (float32; int16 PCM with `device_backend`, or
        when it asked for `remove_silence`); one whose text is a list of chunk texts (a streamed request's head or tail) gets its per-chunk
        waves, for the caller's `infer.StreamJoiner`.  `infer.finish_requests` does the joining, on the device with `device_backend`."""
        finish = dict(device_backend=self.device_backend, want="pcm16" if self.device_backend else "float")
        with self._device_lock:
            return infer.infer_requests(requests, self.model_obj, self.vocoder, mel_spec_type=self.mel_spec_type, finish=finish, **self.opts)

    def close(self):
        """Unload: stop the batcher (requests already queued are served, later ones refused) and drop the model objects."""
        if self.batcher is not None:
            self.batcher.close()
            self.batcher = None
        closer = getattr(self.model_obj, "close", None)
        if callable(closer):
            closer()                             # ShardedSampler: releases the worker ranks
        self.model = self.model_obj = self.vocoder = None

    def _decode_flac(self, data):
        """`load_audio`'s FLAC reader for this manager: what needs no samples is refused first (`flac_stream_info`: the metadata chain,
        STREAMINFO's limits, the cap), then the stream is decoded on the device under the device lock -- or, without `device_decode` or
        without a loaded model's device, by `read_flac`."""
        import torch
        infer.wave_codec.flac_stream_info(data)
        model_obj = getattr(self.model_obj, "local", self.model_obj)
        device = getattr(model_obj, "device", None)
        if not self.device_decode or device is None or torch.device(device).type != "cuda":
            return infer.read_flac(data)
        from . import ops
        with self._device_lock:
            return ops.flac_decode([data], device=device)[0]

    def decode_audio(self, src):
        """(float32 wave [channels, n], sample_rate) of an upload or a recording -- a path, the file's bytes or a binary file object; WAV
        or native FLAC (`infer.load_audio`), FLAC through `_decode_flac`.  ValueError for anything unreadable."""
        return infer.load_audio(src, flac=self._decode_flac)

    def _voice(self, ref_audio_path, ref_text):
        """Once per voice: the reference's pre-step (clip to 15 s / trim silence, `preprocess_ref_audio_text`), then the prologue of
        every `infer_process` call for it (mono, rms gain, 24 kHz) and -- on first use -- its mel on the device."""
        key = (ref_audio_path, ref_text)
        with self._prep_lock:
            if key not in self._prep_cache:
                wav_path, ref_text_n = infer.preprocess_ref_audio_text(ref_audio_path, ref_text, show_info=lambda *_: None)
                self._prep_cache[key] = (infer.PreparedVoice(wav_path), ref_text_n)
            return self._prep_cache[key]

    @staticmethod
    def _request(voice, ref_text, text, opts):
        """The batcher's request tuple: (voice, ref_text, text), plus the request's options when it sets any (`infer.infer_requests`)."""
        return (voice, ref_text, text, opts) if opts else (voice, ref_text, text)

    def _call(self, text, ref_audio_path, ref_text, **options):
        return self._serve(lambda: self._voice(ref_audio_path, ref_text), text, options)

    def _clip_voice(self, ref_audio, ref_text, clip_short=True, denoise=False):
        """(PreparedVoice, normalised ref_text) of an uploaded clip -- WAV bytes or a (wave [ch, n], sr) pair -- prepared once per
        (content, ref_text, clip_short, denoise) and kept in the LRU cache: the same upload with and without `denoise` are two voices.  Host work only: read, quantise to int16 (16-bit PCM passes through bit for
        bit; any other format as clip(round(x * 32768), -32768, 32767) -- pydub would hand those to ffmpeg), the silence pre-step
        (`audio_prep.preprocess_ref_segment`), back to float32.  With `device_frontend` the voice is deferred: its mono mix / gain /
        resampling run on the device with the batch it first rides in; with `device_prestep` as well the int16 frames go through
        `ops.ref_prestep` under the device lock and the clip never returns to the host.  Everything that can be refused is refused here with
        ValueError, before anything is queued: an empty `ref_text`, an unreadable WAV, a rate below 11 025 Hz, non-finite samples, a clip
        that is empty or all-zero after the pre-step, a rate pair whose tap table is refused, a `denoise` that is not a bool or whose clip is
        longer than `audio_prep.DENOISE_MAX_SAMPLES` at 24 kHz.  `denoise` (`infer.PreparedVoice`) acts behind the front-end: the silence
        pre-step still sees the recording as it was uploaded."""
        return self._clip_voices([(ref_audio, ref_text, clip_short, denoise)])[0]

    def _prestep_device(self):
        """The device `ops.ref_prestep` runs on, or None where the host pre-step runs: `device_prestep` needs `device_frontend` and a model on a GPU."""
        import torch
        if not (self.device_prestep and self.device_frontend):
            return None
        device = getattr(getattr(self.model_obj, "local", self.model_obj), "device", None)
        return device if device is not None and torch.device(device).type == "cuda" else None

    def _clip_pcm(self, ref_audio):
        """(int16 frames [n, channels], sample_rate) of an upload: read, check, quantise."""
        import torch
        if isinstance(ref_audio, tuple):
            wave, sr = ref_audio[0].detach().cpu().to(torch.float32), int(ref_audio[1])
        else:
            try:
                wave, sr = self.decode_audio(ref_audio)
            except ValueError as e:
                raise ValueError(f"Invalid audio: {e}") from e
        if wave.dim() != 2 or wave.shape[0] < 1:
            raise ValueError(f"Invalid audio: expected [channels, samples] (got {tuple(wave.shape)})")
        x = wave.numpy()
        if not np.isfinite(x).all():
            raise ValueError("Invalid audio: the clip has non-finite samples.")
        pcm = np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
        return np.ascontiguousarray(pcm.T), sr

    def _prestep_clips(self, new, audios, device):
        """The silence pre-step of the new uploads `new` (keys whose third element is `clip_short`; `audios[key]`: the upload) -> key ->
        (float32 clip [ch, n], sample_rate): on `device` (`_prestep_device`) ONE `ops.ref_prestep` call per distinct sample rate, else
        `audio_prep.preprocess_ref_segment` on the host.  ValueError for an unreadable, non-finite, empty or silent clip."""
        import torch
        clips, by_rate = {}, {}
        for key in new:
            pcm, sr = self._clip_pcm(audios[key])
            if device is not None and sr >= 11025 and sr * pcm.shape[1] < 2 ** 23:      # (beyond that the device's exact window sums end)
                by_rate.setdefault(sr, []).append((key, pcm))
                continue
            seg = audio_prep.preprocess_ref_segment(audio_prep.PcmSegment(pcm, sr), key[2], show_info=lambda *_: None)
            if seg.frames.shape[0] == 0 or not seg.frames.any():
                raise ValueError("Invalid audio: the clip is empty or silent.")
            clips[key] = (torch.from_numpy(np.ascontiguousarray((seg.frames.astype(np.float32) / 32768.0).T)), seg.rate)
        if by_rate:
            from . import ops
            for sr, group in by_rate.items():
                n_in, channels = [pcm.shape[0] for _, pcm in group], [pcm.shape[1] for _, pcm in group]
                frames = np.concatenate([pcm.reshape(-1) for _, pcm in group])
                with self._device_lock:
                    packed, lengths, flags = ops.ref_prestep(frames, n_in, channels, sr, [key[2] for key, _ in group], device=device)
                if not all(n > 0 and f for n, f in zip(lengths, flags)):
                    raise ValueError("Invalid audio: the clip is empty or silent.")
                for (key, _), planes in zip(group, ops.ref_prestep_planes(packed, lengths, channels)):
                    clips[key] = (planes, sr)
        return clips

    def _clip_voices(self, specs):
        """`_clip_voice` of several uploads, [(ref_audio, ref_text, clip_short[, denoise])] -> [(PreparedVoice, normalised ref_text)].  The cache is
        looked up per key and every new key is prepared under its own lock (taken in key order, so two callers never wait for each other
        in a ring).  On the host path the new clips are prepared one after the other; with `device_prestep` they share ONE `ops.ref_prestep`
        call per distinct sample rate."""
        import torch
        keys, audios = [], {}
        for ref_audio, ref_text, clip_short, *rest in specs:
            denoise = rest[0] if rest else False
            if not isinstance(denoise, bool):
                raise ValueError(f"denoise must be true or false (got {denoise!r})")
            if not ref_text or not ref_text.strip():
                raise ValueError("Reference text cannot be empty.")
            h = hashlib.sha1()
            if isinstance(ref_audio, tuple):
                arr = np.ascontiguousarray(ref_audio[0].detach().cpu().numpy())
                h.update(repr((arr.shape, str(arr.dtype), int(ref_audio[1]))).encode())
                h.update(arr.tobytes())
            else:
                ref_audio = bytes(ref_audio)
                h.update(ref_audio)
            key = (h.hexdigest(), ref_text, bool(clip_short), denoise)
            keys.append(key)
            audios.setdefault(key, ref_audio)
        results, entries = {}, []
        try:
            for key in sorted(audios):
                with self._clip_lock:
                    if key in self._clip_cache:
                        self._clip_cache.move_to_end(key)
                        results[key] = self._clip_cache[key]
                        continue
                    entry = self._clip_key_locks.setdefault(key, [threading.Lock(), 0])
                    entry[1] += 1
                entries.append((key, entry, [False]))
                entry[0].acquire()
                entries[-1][2][0] = True
                with self._clip_lock:
                    if key in self._clip_cache:      # prepared while this thread waited for the key
                        self._clip_cache.move_to_end(key)
                        results[key] = self._clip_cache[key]
            new = [key for key, _, _ in entries if key not in results]
            device = self._prestep_device() if new else None
            clips = self._prestep_clips(new, audios, device)
            fresh = []
            for key in new:
                clip = clips[key]
                if clip[1] != infer.target_sample_rate:
                    infer.resample_taps(clip[1], infer.target_sample_rate)      # refuses a rate pair it has no table for
                if self.device_frontend:
                    voice = infer.PreparedVoice.deferred(clip, denoise=key[3], reject_marked=self.reject_marked, limits=self.reference_limits)
                else:                                                            # (measured and scored here, before the denoiser)
                    voice = infer.PreparedVoice(clip, denoise=key[3], reject_marked=self.reject_marked, limits=self.reference_limits)
                fresh.append((key, voice))
            if (self.reject_marked is not None or self.reference_limits is not None) and any(voice.pending is not None for _, voice in fresh):
                # the new uploads' front-end now, under the device lock: ONE `ops.ref_assess` and ONE `ops.watermark_detect` call per front-end
                # call measure and score them on its device buffers (`infer.prepare_voices`), and a clip over a limit or a marked clip is
                # refused here -- before it is cached or anything is queued
                with self._device_lock:
                    infer._prepare_deferred([voice for _, voice in fresh], self.model_obj)
            for key, voice in fresh:
                value = (voice, audio_prep.normalize_ref_text(key[1]))
                with self._clip_lock:
                    self._clip_cache[key] = value
                    while len(self._clip_cache) > max(self.clip_cache, 0):
                        self._clip_cache.popitem(last=False)
                results[key] = value
            return [results[key] for key in keys]
        finally:
            for key, entry, held in reversed(entries):
                if held[0]:
                    entry[0].release()
                with self._clip_lock:
                    entry[1] -= 1
                    if entry[1] == 0:
                        self._clip_key_locks.pop(key, None)

    def _serve(self, resolve_voice, text, options, stream=False):
        """What the four `synthesize*` methods do once they know where the voice comes from (`resolve_voice`: `_voice` or `_clip_voice`, called
        after the options are checked): the model must be loaded, `options` go through `request_options` (an unknown name is a ValueError),
        then the request runs -- through the batcher, or alone under the device lock -- or, with `stream`, becomes a `SynthesisStream`: no
        option that needs the whole wave, the first chunk and the remaining chunks as two requests that share one generator when it is seeded
        (the tail's batch runs after the head's: one worker, one batch at a time)."""
        if not self.model:
            raise ValueError("TTS model not loaded")
        opts = self.request_options(**options)
        if stream and stream_refusal(opts):
            raise ValueError(stream_refusal(opts))
        voice, ref_text = resolve_voice()
        if stream:
            chunks = infer.request_chunks(ref_text, voice.seconds, text)
            if "seed" in opts:
                opts["generator"] = infer.request_generator(opts.pop("seed"))
            return self._stream(voice, ref_text, chunks[:1], chunks[1:], opts)
        req = self._request(voice, ref_text, text, opts)
        if self.batcher is not None:   # wait for the batch this request rides in (the route runs in a worker thread, see create_app)
            return self.batcher.submit(req).result(timeout=self.request_timeout_s)
        return self._run_batch([req])[0]

    def synthesize_clip(self, text, ref_audio, ref_text, *, clip_short=True, denoise=False, **options):
        """`synthesize` with the caller's own reference clip instead of a registered voice: `ref_audio` is a WAV file's bytes or a
        (wave [ch, n], sr) pair, `ref_text` its transcript; `clip_short` as in `preprocess_ref_audio_text`; `denoise`: remove stationary
        background noise (hiss, fan noise, hum) from the clip before it is cloned (`audio_prep.denoise_reference`; off unless asked for,
        because a voice without pauses is taken for noise).  The clip never touches the disk (`_clip_voice`); the request then takes the
        same batcher path as `synthesize`, with the same options."""
        return self._serve(lambda: self._clip_voice(ref_audio, ref_text, clip_short, denoise), text, options)

    def synthesize_clip_stream(self, text, ref_audio, ref_text, *, clip_short=True, denoise=False, **options):
        """`synthesize_stream` with an uploaded reference clip (`synthesize_clip`): an iterator of pieces (float32; in the delivery format
        with `sample_rate` / `encoding`) whose concatenation is `synthesize_clip`'s wave given the same noise."""
        return self._serve(lambda: self._clip_voice(ref_audio, ref_text, clip_short, denoise), text, options, stream=True)

    def synthesize(self, text, ref_audio_path, ref_text, **options):
        """The wave of one request.  `options`: any of `infer.REQUEST_OPTIONS`, by keyword -- a name that is not among them is refused by
        `request_options` with ValueError (not the interpreter's TypeError: the four `synthesize*` methods take `**options`).  The sampler
        options (`speed`, `nfe_step`, `cfg_strength`, `sway_sampling_coef`) are this request's own (None: `self.opts`); `seed` draws its noise from its own
        generator (`infer.request_generator`), so the same seeded request gives the same audio whatever it is batched with (shape-invariant
        attention, one GPU).  `ode_method` ("euler", "midpoint", "rk4"; None: the model's): requests of different solvers share a batch, and
        the option reaches the model object only for a request that sets it.  The `infer.DELIVERY_OPTIONS` (`remove_silence`, `loudness`,
        `sample_rate`, `encoding`, `flac_level`) and the `infer.PROSODY_OPTIONS` (`tempo`: the duration divided by it at the same pitch, where
        `speed` asks the sampler for another take; `pitch`: whole semitones at the same duration; see `infer.WaveSpec`) and, beside a non-zero
        `pitch`, `keep_formants` (the voice's formants stay where they were: `infer.psola_pcm16`) make the result
        `infer.finish_pcm16` of the wave's int16 PCM --
        computed on the device with `device_backend`, where every result is int16 PCM, and the same bytes either way."""
        if not self.model:
            raise ValueError("TTS model not loaded")
        return self.model(text, ref_audio_path=ref_audio_path, ref_text=ref_text, **options)   # (`_call`, which checks the options)

    def synthesize_stream(self, text, ref_audio_path, ref_text, **options):
        """`synthesize` as an iterator of float32 pieces (24 kHz) whose concatenation is `synthesize`'s wave given the same noise (see
        `infer.infer_process_stream`).  The request's first chunk is synthesized on its own and its stable samples come out as soon as it is
        done; the remaining chunks follow as a second request.  With a micro-batcher the first chunk rides in the next batch and the
        remaining chunks are queued once that batch has started, so they ride in a later one; without, the two run one after the other,
        each under the device lock (released in between).  Closing the iterator early (client disconnect) cancels the remaining chunks
        if their batch has not started.  Errors about the model or the voice are raised here, not on the first `next()`.  Options as in
        `synthesize`; with a `seed`, the first chunk and the remaining chunks draw from the request's one generator in chunk order, so the
        pieces equal `synthesize`'s wave with that seed.  The remaining chunks keep the first chunk's `ode_method`.  With `sample_rate` /
        `encoding` the pieces come in the delivery format, each float32 piece through an `infer.StreamDelivery` on the host (int16 at that
        rate, uint8 code bytes, or for "flac" the 42-byte stream header with the totals unknown and then the frames as they complete), and
        their concatenation equals `synthesize`'s result with the same options byte for byte (for "flac": behind the header, and both decode
        to the same samples).  The header comes from the first `next()` once the first chunk is synthesized, so a failing first chunk raises
        there before any byte.  `remove_silence`, `loudness`, `tempo` and `pitch` need the whole wave: ValueError."""
        return self._serve(lambda: self._voice(ref_audio_path, ref_text), text, options, stream=True)

    def _stream(self, voice, ref_text, head, tail, opts=None):
        spec = infer.WaveSpec.of(opts or {})   # the delivery format is applied here, piece by piece: the head and tail requests stay plain
        opts = {k: v for k, v in (opts or {}).items() if k not in infer.WAVE_OPTIONS}
        return self._stream_requests(self._request(voice, ref_text, head, opts), self._request(voice, ref_text, tail, opts) if tail else None, spec)

    def _stream_requests(self, head_request, tail_request, spec, tail_pieces=None):
        """A stream of two requests: the head's chunk waves, then (unless None) the tail's, through one `infer.StreamJoiner` and, unless
        `spec` has the plain format, an `infer.StreamDelivery`.  `tail_pieces(joiner, result)`: the pieces the tail's result releases
        (default: its chunk waves pushed in order; a script cuts the joiner between its segments)."""
        lock, state = threading.Lock(), {"closed": False, "tail": None, "error": None}
        started = threading.Event()
        tail = tail_request is not None
        if tail_pieces is None:
            def tail_pieces(joiner, waves):
                return joiner.pieces(waves)

        def submit_tail():                        # on the batcher's thread, once the head's batch has formed
            with lock:
                try:
                    if not state["closed"]:
                        state["tail"] = self.batcher.submit(tail_request)
                except Exception as e:    # noqa: BLE001 -- e.g. the batcher is closing: reported to the consumer
                    state["error"] = e
            started.set()

        def cancel():
            with lock:
                state["closed"] = True
                if state["tail"] is not None:
                    state["tail"].cancel()        # a no-op once its batch has started or it is done

        def pieces():
            joiner = infer.StreamJoiner(infer.cross_fade_duration)
            try:
                if self.batcher is not None:
                    head_f = self.batcher.submit(head_request, on_start=submit_tail if tail else None)
                    head_waves = head_f.result(timeout=self.request_timeout_s)
                else:
                    head_waves = self._run_batch([head_request])[0]
                yield from joiner.pieces(head_waves)
                if tail:
                    if self.batcher is not None:
                        started.wait(timeout=self.request_timeout_s)
                        if state["error"] is not None:
                            raise state["error"]
                        if state["tail"] is None:     # closed before the tail was queued
                            return
                        tail_waves = state["tail"].result(timeout=self.request_timeout_s)
                    else:
                        tail_waves = self._run_batch([tail_request])[0]
                    yield from tail_pieces(joiner, tail_waves)
                yield from joiner.pieces(flush=True)
            finally:                              # normal end, error, or the consumer closed the stream
                cancel()

        def delivered():
            delivery, gen = infer.StreamDelivery(spec), pieces()
            try:
                for piece in gen:
                    yield from delivery.feed(piece)
                yield from delivery.finish()
            finally:
                gen.close()

        return SynthesisStream(pieces() if spec.plain_format else delivered(), cancel)

    def _script_segments(self, text, voices, gap):
        """The host part of a script request, every refusal a ValueError before anything is queued: `voices` needs "main", `text` at least
        one non-empty piece and at most `infer.MAX_SCRIPT_SEGMENTS` (`infer.split_voice_tags`), `gap` its range; then each voice the text
        uses is resolved once -- a registered one by `_voice`, an uploaded one by `_clip_voice` (its SHA-1 LRU, deferred with
        `device_frontend`: the new clips of the script are then prepared in the ONE front-end call of the batch the script rides in; with
        `device_prestep` the uploads are resolved together, `_clip_voices`: one `ops.ref_prestep` call per distinct rate).
        Returns [(voice, ref_text, piece text, speed | None)]."""
        if not isinstance(voices, dict) or "main" not in voices:
            raise ValueError('voices needs a "main" entry')
        if not isinstance(text, str) or not text.strip():
            raise ValueError("Text to synthesize cannot be empty.")
        pieces = infer.split_voice_tags(text, voices)
        if not pieces:
            raise ValueError("Text to synthesize cannot be empty.")
        if len(pieces) > infer.MAX_SCRIPT_SEGMENTS:
            raise ValueError(f"a script needs between 1 and {infer.MAX_SCRIPT_SEGMENTS} pieces (got {len(pieces)})")
        infer.check_script_gap(gap)
        resolved, uploads, together = {}, [], self._prestep_device() is not None
        for tag in dict.fromkeys(tag for tag, _ in pieces):
            spec = dict(voices[tag])
            unknown = set(spec) - {"ref_audio_path", "ref_audio", "ref_text", "clip_short", "denoise", "speed"}
            if unknown or ("ref_audio_path" in spec) == ("ref_audio" in spec):
                raise ValueError(f"voice {tag!r}: give ref_audio_path or ref_audio, ref_text and optionally clip_short, speed, denoise "
                                 f"(got {sorted(spec)})")
            if "denoise" in spec and not isinstance(spec["denoise"], bool):
                raise ValueError(f"voice {tag!r}: denoise must be true or false (got {spec['denoise']!r})")
            if "denoise" in spec and "ref_audio_path" in spec:
                raise ValueError(f"voice {tag!r}: denoise is an option of an uploaded clip (ref_audio), not of a registered voice")
            speed = self.request_options(("speed",), speed=spec.get("speed")).get("speed")
            if not spec.get("ref_text") or not spec["ref_text"].strip():
                raise ValueError("Reference text cannot be empty.")
            if "ref_audio_path" in spec:
                voice, ref_text = self._voice(spec["ref_audio_path"], spec["ref_text"])
            elif together:
                uploads.append((tag, speed, (spec["ref_audio"], spec["ref_text"], spec.get("clip_short", True), spec.get("denoise", False))))
                continue
            else:
                voice, ref_text = self._clip_voice(spec["ref_audio"], spec["ref_text"], spec.get("clip_short", True), spec.get("denoise", False))
            resolved[tag] = (voice, ref_text, speed)
        if uploads:                                  # the script's uploads together: one pre-step call per distinct rate for the new ones
            for (tag, speed, _), (voice, ref_text) in zip(uploads, self._clip_voices([u for _, _, u in uploads])):
                resolved[tag] = (voice, ref_text, speed)
        return [(resolved[tag][0], resolved[tag][1], piece, resolved[tag][2]) for tag, piece in pieces]

    def synthesize_script(self, text, voices, *, gap=0.0, **options):
        """A multi-voice script (F/infer/infer_cli.py:166-208) as ONE request: `text` with `[tag]` marks (`infer.split_voice_tags`: a piece
        without a known tag is spoken by "main"), `voices` = {tag: dict(ref_audio_path=..., ref_text=...) | dict(ref_audio=<WAV bytes or
        (wave, sr)>, ref_text=..., clip_short=True, denoise=False)}, each with an optional `speed`; `gap`: seconds of silence between pieces (0 to 5).
        `options`: `infer.REQUEST_OPTIONS` as in `synthesize`, for the whole script -- one `seed` for all its chunks in order, and
        `remove_silence` / `loudness` / `sample_rate` / `encoding` on the joined wave (so two voices of different prompt levels come out at one programme loudness).  The script is one item of its batch (`infer.ScriptRequest`): its
        pieces are sampled and vocoded with everything else in the batch, cross-faded inside a piece and concatenated between pieces
        (`infer.join_segments`) -- with `device_backend` in the batch's single `ops.wave_finish_joins` call, as int16 PCM."""
        return self._script(text, voices, gap, options)

    def synthesize_script_stream(self, text, voices, *, gap=0.0, **options):
        """`synthesize_script` as an iterator of pieces whose concatenation is its wave given the same noise: the head is the first chunk
        of the first piece, the tail the rest of the script as one request of per-chunk texts; the joiner is cut between pieces
        (`infer.StreamJoiner.cut`).  Delivery format and `remove_silence` as in `synthesize_stream`."""
        return self._script(text, voices, gap, options, stream=True)

    def _script(self, text, voices, gap, options, stream=False):
        if not self.model:
            raise ValueError("TTS model not loaded")
        opts = self.request_options(**options)
        if stream and stream_refusal(opts):
            raise ValueError(stream_refusal(opts))
        segments = self._script_segments(text, voices, gap)
        if not stream:
            req = infer.ScriptRequest(segments, opts, gap)
            if self.batcher is not None:
                return self.batcher.submit(req).result(timeout=self.request_timeout_s)
            return self._run_batch([req])[0]
        if "seed" in opts:
            opts["generator"] = infer.request_generator(opts.pop("seed"))
        spec = infer.WaveSpec.of(opts)            # (applied to the pieces, as in `_stream`)
        opts = {k: v for k, v in opts.items() if k not in infer.WAVE_OPTIONS}
        chunked = [(voice, ref_text, infer.request_chunks(ref_text, voice.seconds, piece), speed) for voice, ref_text, piece, speed in segments]
        voice, ref_text, chunks, speed = chunked[0]
        head = self._request(voice, ref_text, chunks[:1], dict(opts, speed=speed) if speed is not None else opts)
        continues = len(chunks) > 1                   # the tail's first segment is the rest of the head's piece: no cut in front of it
        rest = ([(voice, ref_text, chunks[1:], speed)] if continues else []) + chunked[1:]
        gap_samples = int(float(gap) * infer.target_sample_rate)

        def tail_pieces(joiner, per_segment):
            for k, waves in enumerate(per_segment):
                if k or not continues:
                    yield from joiner.pieces(cut=True)
                    if gap_samples:
                        yield from joiner.pieces([np.zeros(gap_samples, dtype=np.float32)], cut=True)
                yield from joiner.pieces(waves)

        return self._stream_requests(head, infer.ScriptRequest(rest, opts, gap) if rest else None, spec, tail_pieces)

    def edit(self, audio, target_text, parts_to_edit, fix_duration=None, *, nfe_step=None, cfg_strength=None, sway_sampling_coef=None,
             seed=None, ode_method=None, sample_rate=None, encoding=None, loudness=None, flac_level=None, watermark=None):
        """Speech editing (`infer.speech_edit`, F/infer/speech_edit.py): regenerate `parts_to_edit` of the recording `audio` (a path, WAV
        bytes or a (tensor, sr) pair) so that it speaks `target_text`, with this manager's sampler settings unless the call sets its own
        (`seed`: the edit's noise from its own generator; `ode_method`: the edit's solver, handed on only when set).  The host preparation runs outside the device lock, the sampler and vocoder
        under it (not through the micro-batcher); with a `ShardedSampler` on rank 0's own model.  Returns the wave (float32, 24 kHz) -- with
        any of `sample_rate`, `encoding`, `loudness` and `flac_level` (`infer.WaveSpec`), or with a `watermark` key (the manager's unless the
        call names one: the whole returned recording is marked, kept parts included), `infer.finish_pcm16` of its int16 PCM on the host."""
        if not self.model:
            raise ValueError("TTS model not loaded")
        opts = dict(self.opts, **self.request_options(EDIT_OPTIONS, nfe_step=nfe_step, cfg_strength=cfg_strength,
                                                      sway_sampling_coef=sway_sampling_coef, seed=seed, ode_method=ode_method))
        delivery = self.request_options(EDIT_DELIVERY, sample_rate=sample_rate, encoding=encoding, flac_level=flac_level, loudness=loudness)
        spec = infer.WaveSpec.of(dict(delivery, **self.request_options(EDIT_MARK, watermark=watermark)))
        model_obj = getattr(self.model_obj, "local", self.model_obj)
        # host work (read, mono mix, resample, plan, tokens) and every rejection happen before the device lock is taken (a FLAC recording is
        # decoded under it with `device_decode`, after everything that needs no samples has been refused)
        if not isinstance(audio, tuple):
            audio = self.decode_audio(audio)
        prep = infer.prepare_edit(audio, target_text, parts_to_edit, fix_duration, mel_spec_type=self.mel_spec_type)
        extra = dict(generators=[infer.request_generator(opts["seed"])]) if opts.get("seed") is not None else {}
        if opts.get("ode_method") is not None:
            extra["ode_method"] = opts["ode_method"]
        with self._device_lock:
            (wave, _, _), = infer.speech_edit_batch([prep], model_obj, self.vocoder, mel_spec_type=self.mel_spec_type,
                                                    nfe_step=opts["nfe_step"], cfg_strength=opts["cfg_strength"],
                                                    sway_sampling_coef=opts["sway_sampling_coef"], **extra)
        wave = np.asarray(wave, dtype=np.float32)
        if not spec.needs_whole_wave():   # (nothing named, no mark: the float wave)
            return wave
        return infer.finish_pcm16(infer.quantise_pcm16(wave), spec)

    def detect_watermark(self, audio, keys=None) -> list:
        """Whether a recording carries a mark: one `infer.WatermarkScore(key, z, offset, detected)` per key for `audio` -- a path, WAV or FLAC
        bytes, or a (wave [ch, n], sr) pair --, read the way a reference upload is read: `decode_audio`, mono mix, sinc resampling to 24 kHz
        (`infer.resample_sinc_hann`).  `keys`: 1 to 16 keys; None: this manager's own `watermark`.  ValueError when neither is given, for a bad
        key and for audio that cannot be read.  Host arithmetic in fp64 (`infer.detect_watermark`)."""
        keys, mono = self._watermark_clip("detect_watermark", audio, keys)
        return infer.detect_watermark(mono, keys)

    def _watermark_clip(self, what, audio, keys):
        """(keys, the recording as mono 24 kHz fp32 [n]) of `detect_watermark` and `read_watermark`."""
        import torch
        if keys is None:
            if self.watermark is None:
                raise ValueError(f"{what} needs keys: this manager has no watermark key of its own")
            keys = [infer.watermark_key(self.watermark)]
        keys = infer.check_watermark_keys(keys)
        wave, sr = audio if isinstance(audio, tuple) else self.decode_audio(audio)
        wave = torch.as_tensor(wave, dtype=torch.float32)
        if wave.dim() == 1:
            wave = wave[None]
        if wave.dim() != 2 or wave.shape[0] < 1:
            raise ValueError(f"Invalid audio: expected [channels, samples] (got {tuple(wave.shape)})")
        mono = wave.mean(dim=0, keepdim=True)
        if int(sr) != infer.target_sample_rate:
            mono = infer.resample_sinc_hann(mono, int(sr), infer.target_sample_rate)
        return keys, mono[0].numpy()

    def read_watermark(self, audio, keys=None) -> list:
        """Which request a recording came from: one `infer.WatermarkRead(key, z, offset, detected, id, id_z)` per key -- `detect_watermark`'s
        score and the trace id the key's mark carries (None when the key is not detected or a symbol stays below
        `infer.WATERMARK_ID_THRESHOLD`) with the smallest symbol score.  `audio` and `keys` as `detect_watermark`'s.  With `device_frontend` and
        a model on a GPU the clip is read there, the way uploads are scored for `reject_marked`: ONE `ops.watermark_read_ids` call per four
        keys under the device lock, fp32; otherwise on the host in fp64 (`infer.read_watermark`)."""
        import torch
        keys, mono = self._watermark_clip("read_watermark", audio, keys)
        device = getattr(getattr(self.model_obj, "local", self.model_obj), "device", None)
        if not (self.device_frontend and device is not None and torch.device(device).type == "cuda") or not np.isfinite(mono).all():
            return infer.read_watermark(mono, keys)              # (a sample that is not finite is the host's ValueError)
        from . import ops
        n, most, out = min(len(mono), infer.WATERMARK_MAX_SAMPLES), infer.WATERMARK_ID_KEYS_MAX, []
        with self._device_lock:
            wave = torch.from_numpy(mono[:n].copy()).to(device)
            rows = [ops.watermark_read_ids(wave, [0], [n], ops.watermark_tag_carriers(keys[at:at + most], wave.device)) for at in range(0, len(keys), most)]
            rows = torch.cat(rows, dim=1)[0].cpu().numpy()
        return ops.watermark_reads(rows, keys)

    def scan_watermark(self, audio, keys=None) -> list:
        """Where a long or spliced recording carries a mark, and whose: one `infer.WatermarkSpan(key, start, end, z, offset, id, id_z)` per
        marked stretch and key, start and end in samples at 24 kHz, sorted by (start, the key's position) -- `infer.scan_watermark`, which
        folds windows of two periods instead of the whole clip, so stretches cut together are told apart and nothing is cut at 60 s.
        `audio` and `keys` as `detect_watermark`'s.  ValueError for a recording over 600 s (never truncated).  With `device_frontend` and a
        model on a GPU the recording is scanned there under the device lock (`ops.watermark_scan`: one call over every window, then at most
        one per four keys over the spans, fp32); otherwise on the host in fp64."""
        import torch
        keys, mono = self._watermark_clip("scan_watermark", audio, keys)
        device = getattr(getattr(self.model_obj, "local", self.model_obj), "device", None)
        if (not (self.device_frontend and device is not None and torch.device(device).type == "cuda") or len(mono) > infer.WATERMARK_SCAN_MAX_SAMPLES
                or not np.isfinite(mono).all()):
            return infer.scan_watermark(mono, keys)              # (too long, or a sample that is not finite: the host's ValueError)
        if len(mono) < infer.WATERMARK_MIN_SAMPLES:
            return []
        from . import ops
        with self._device_lock:
            return ops.watermark_scan(torch.from_numpy(np.ascontiguousarray(mono)).to(device), keys)

    def check_reference(self, audio, clip_short=True):
        """The `infer.ReferenceReport` of a would-be reference clip -- WAV or FLAC bytes, or a (wave [ch, n], sr) pair -- taken through
        `decode_audio`, the silence pre-step and the front-end exactly as a clone upload is (`_clip_voice`; with `device_frontend` and a
        loaded model the front-end and one `ops.ref_assess` call run on the device under the device lock), but neither cached nor gated:
        `reference_problems` lists what this manager's limits would refuse.  ValueError for what the clone route refuses as unreadable."""
        key = ("", "", bool(clip_short), False)
        audio = audio if isinstance(audio, tuple) else bytes(audio)
        clip = self._prestep_clips([key], {key: audio}, self._prestep_device())[key]
        if clip[1] != infer.target_sample_rate:
            infer.resample_taps(clip[1], infer.target_sample_rate)
        if not self.device_frontend:
            return infer.PreparedVoice(clip, assess=True).report
        voice = infer.PreparedVoice.deferred(clip, assess=True)
        with self._device_lock:
            infer._prepare_deferred([voice], self.model_obj)
        return voice.report

    def reference_problems(self, report, denoise=False) -> list:
        """What `reference_limits` would refuse `report` for, one sentence per violated limit; empty without limits."""
        return infer.reference_problems(report, self.reference_limits, denoise)


class HTTPError(Exception):
    """Carries (status_code, detail) out of `synthesize_speech`; the route turns it into fastapi.HTTPException."""

    def __init__(self, status_code: int, detail: str):
        super().__init__(detail)
        self.status_code, self.detail = status_code, detail


def _checked_voice(registry: VoiceRegistry, text: str, ref_audio_name: str, ref_text: str | None):
    """The checks of `S/utils/tts_utils.py:38-65`, in its order and with its messages: (voice, ref_text), the voice's own transcript
    when the request brings none."""
    voice = registry.get(ref_audio_name)
    if voice is not None and not ref_text:
        ref_text = voice.ref_text
    if voice is None:
        raise HTTPError(400, "Invalid reference audio name.")
    if not text.strip():
        raise HTTPError(400, "Text to synthesize cannot be empty.")
    if not ref_text or not ref_text.strip():
        raise HTTPError(400, "Reference text cannot be empty.")
    return voice, ref_text


RESPONSE_FORMATS = {"wav": "audio/wav", "pcm": "audio/pcm"}   # response_format -> media type; "pcm": headerless samples / code bytes
MEDIA_TYPES = dict(RESPONSE_FORMATS, flac="audio/flac")       # container -> media type: FLAC (`encoding: "flac"`) is its own container


def check_response_format(response_format) -> str:
    """"wav" (None: the default) or "pcm"; anything else is a ValueError the routes return as 400."""
    fmt = "wav" if response_format is None else response_format
    if not isinstance(fmt, str) or fmt not in RESPONSE_FORMATS:
        raise ValueError(f"response_format must be one of {', '.join(repr(f) for f in RESPONSE_FORMATS)} (got {response_format!r})")
    return fmt


def container_format(response_format, encoding=None) -> str:
    """The container of a response body: `check_response_format`'s "wav" or "pcm" -- or "flac" for `encoding` "flac", which is its own
    container: `response_format` must then be absent (ValueError, a 400 on the routes, for "wav" or "pcm" beside it)."""
    if encoding not in infer.FLAC_ENCODINGS:
        return check_response_format(response_format)
    if response_format is not None:
        check_response_format(response_format)
        raise ValueError(f'encoding "flac" is its own container (audio/flac): response_format must be absent (got {response_format!r})')
    return "flac"


def response_body(audio, options: dict, response_format: str = "wav") -> io.BytesIO:
    """The response body of a request's result in the delivery format its `options` name: a WAV file (`wav_bytes`), with "pcm" the
    headerless little-endian samples / code bytes, and for `encoding` "flac" the FLAC stream the result holds."""
    rate, enc = infer.delivery_format(options.get("sample_rate"), options.get("encoding"))   # (the format alone: checked or not, nothing else of them counts here)
    return io.BytesIO(delivery_bytes(audio, enc)) if enc in infer.FLAC_ENCODINGS or response_format == "pcm" else wav_bytes(audio, rate, enc)


def synthesize_speech(tts_manager: TTSManager, registry: VoiceRegistry, text: str, ref_audio_name: str, ref_text: str | None,
                      response_format: str = "wav", **options):
    """`S/utils/tts_utils.py:38-65` with the same checks in the same order and the same messages; `options` go to `TTSManager.synthesize`,
    and the body comes in the delivery format they name (`response_body`)."""
    voice, ref_text = _checked_voice(registry, text, ref_audio_name, ref_text)
    audio = tts_manager.synthesize(text, ref_audio_path=voice.audio_path, ref_text=ref_text, **options)
    return response_body(audio, options, response_format)


def stream_speech(tts_manager: TTSManager, registry: VoiceRegistry, text: str, ref_audio_name: str, ref_text: str | None, **options):
    """`synthesize_speech`'s checks, then `TTSManager.synthesize_stream`: an iterator of float32 pieces."""
    voice, ref_text = _checked_voice(registry, text, ref_audio_name, ref_text)
    return tts_manager.synthesize_stream(text, ref_audio_path=voice.audio_path, ref_text=ref_text, **options)


def request_models():
    """The routes' request models by name (`create_app`): pydantic is imported here, on first use, like fastapi is there."""
    from pydantic import BaseModel, ConfigDict

    class SamplerFields(BaseModel):                  # per-request sampler settings; None = the manager's (TTSManager.opts)
        nfe_step: int | None = None
        cfg_strength: float | None = None
        sway_sampling_coef: float | None = None
        seed: int | None = None
        ode_method: str | None = None
        sample_rate: int | None = None               # the delivery format (infer.deliver_pcm16); None = 24 kHz 16-bit PCM in a WAV
        encoding: str | None = None
        loudness: float | None = None                # programme loudness target in LUFS (infer.normalise_loudness_pcm16); None = the level as synthesized
        flac_level: typing.Any = None                # 0 or 1 beside encoding "flac" (infer.check_flac_level); untyped, so that true and "1" arrive as sent and are refused
        response_format: str | None = None

    class SpeechFields(SamplerFields):               # what the three speech routes take on top: with SamplerFields, every infer.REQUEST_OPTIONS name
        speed: float | None = None
        remove_silence: bool | None = None
        tempo: typing.Any = None                     # 0.5 to 2 in steps of 0.01: the duration divided by it, the pitch kept (infer.shift_pcm16); untyped like flac_level
        pitch: typing.Any = None                     # whole semitones, -6 to 6, the duration kept; untyped, so that true and 2.0 arrive as sent and are refused
        watermark: typing.Any = None                 # the key of a provenance mark, 1 to 2^48 - 1, or {"key": K, "id": I} with a trace id (infer.mark_pcm16); untyped, so that true, 1.0 and "1" are refused
        keep_formants: typing.Any = None             # true beside a non-zero pitch: the voice's formants stay where they were (infer.psola_pcm16); untyped, so that 1 and "true" are refused

    class KannadaSynthesizeRequest(SpeechFields):    # S/utils/tts_utils.py:27-28
        text: str
        stream: bool = False

    class SynthesizeRequest(SpeechFields):           # S/utils/tts_utils.py:22-25
        text: str
        ref_audio_name: str
        ref_text: str | None = None
        stream: bool = False

    class EditRequest(SamplerFields):                # F/infer/speech_edit.py's inputs; JSON (base64 WAV), not multipart
        audio: str
        text: str
        parts_to_edit: list[list[float]]
        fix_duration: list[float] | None = None
        denoise: typing.Any = None                   # not an option of this route (an edit keeps the recording): anything but an absent field is a 400
        watermark: typing.Any = None                 # the key of a provenance mark on the whole returned recording (serve.EDIT_MARK)

    class CloneRequest(SpeechFields):                # zero-shot cloning from the caller's own clip; JSON (base64 WAV), not multipart
        text: str
        ref_audio: str
        ref_text: str
        clip_short: bool = True
        denoise: bool = False                        # remove stationary background noise from the clip (audio_prep.denoise_reference)
        stream: bool = False

    class ScriptVoice(BaseModel):                    # one voice of a script: a registered name, or the caller's own clip (base64 WAV)
        ref_audio_name: str | None = None
        ref_audio: str | None = None
        ref_text: str | None = None
        clip_short: bool = True
        speed: float | None = None
        model_config = ConfigDict(extra="allow")     # `denoise` (true / false, of an uploaded clip only) is read from the extras: `_run_script`

    class ScriptRequest(SpeechFields):               # F/infer/infer_cli.py:166-208: `[tag]` text and a voices table; JSON, not TOML
        text: str
        voices: dict[str, ScriptVoice]
        gap: float = 0.0
        stream: bool = False

    class DetectRequest(BaseModel):                  # `/v1/audio/watermark/detect`: a recording (base64 WAV or FLAC) and the keys to score it against
        audio: str
        keys: typing.Any = None                      # 1 to 16 keys; absent: the manager's own.  Untyped, so that a bad key arrives as sent and is refused
        ids: typing.Any = None                       # true: also read the trace id each key's mark carries (TTSManager.read_watermark)

    class ScanRequest(BaseModel):                    # `/v1/audio/watermark/scan`: a long or spliced recording (base64 WAV or FLAC) and the keys to look for
        audio: str
        keys: typing.Any = None                      # 1 to 16 keys; absent: the manager's own.  Untyped, as DetectRequest's

    class ReferenceCheckRequest(BaseModel):          # `/v1/audio/reference/check`: a would-be reference clip (base64 WAV or FLAC)
        audio: str
        clip_short: bool = True

    return types.SimpleNamespace(KannadaSynthesizeRequest=KannadaSynthesizeRequest, SynthesizeRequest=SynthesizeRequest, CloneRequest=CloneRequest,
                                 EditRequest=EditRequest, ScriptRequest=ScriptRequest, ScriptVoice=ScriptVoice, DetectRequest=DetectRequest,
                                 ReferenceCheckRequest=ReferenceCheckRequest, ScanRequest=ScanRequest)


def create_app(tts_manager: TTSManager, registry: VoiceRegistry):
    """FastAPI app with the reference's `/v1/audio/speech` route (`S/routes/speech.py:19-41`) and `/v1/audio/edit` (speech editing:
    JSON body {"audio": base64 WAV, "text": the full new transcript, "parts_to_edit": [[start_s, end_s], ...], "fix_duration": [...] | null}
    -> the edited recording as WAV), plus `/v1/audio/speech/clone`: `/v1/audio/speech/voice` with the caller's own reference clip
    ({"text", "ref_audio": base64 WAV, "ref_text", "clip_short": true, "denoise": false, ...}) instead of a registered voice's name
    (`denoise`: remove stationary background noise from the clip first; an input-side option, so it works with `"stream": true`; the edit
    route and the routes on registered voices do not take it), and
    `/v1/audio/speech/script`: a multi-voice script ({"text": "[main] ... [town] ...", "voices": {tag: {"ref_audio_name" | "ref_audio":
    base64 WAV, "ref_text", "clip_short"?, "denoise"?, "speed"?}}, "gap": seconds between pieces, ...}) as one request.  The speech routes take `"stream": true`: the WAV then arrives chunk by chunk (`_run_stream`), its
    PCM samples identical to the unstreamed response's.  Every route also takes the optional sampler fields `nfe_step`, `cfg_strength`,
    `sway_sampling_coef`, `seed`, `ode_method` ("euler", "midpoint" or "rk4": the request's ODE solver) and (speech routes) `speed` and
    `remove_silence` (true: pauses of 1 s or more are cut down to 500 ms on each side; 400 together with `"stream": true`), checked
    before anything is queued (400 with `check_request_options`'s message); an omitted field is the manager's setting (`ode_method`: the
    model's).  With a `seed`, the same request returns the same audio.  Every route takes `sample_rate`, `encoding`, `flac_level` and
    `loudness` as `infer.WaveSpec` describes them (a bad value or combination is a 400; `loudness` is measured on the whole wave, so it is
    a 400 together with `"stream": true`: `STREAM_LOUDNESS`), the speech routes also `tempo` (0.5 to 2: the duration divided by it, the pitch
    kept) and `pitch` (whole semitones, -6 to 6, the duration kept), applied to the finished wave (`infer.shift_pcm16`; 400 together with
    `"stream": true`: `STREAM_PROSODY`; not on the edit route, which keeps the recording's timing) and beside a non-zero `pitch` `keep_formants` (true: the
    pitch moves and the voice's formants stay, `infer.psola_pcm16`; 400 for anything but a bool and without a pitch), every route `watermark` (a key, 1 to 2^48 - 1: the finished wave
    carries that key's provenance mark, `infer.mark_pcm16`; a bad key is a 400, and so is the option together with `"stream": true`:
    `STREAM_WATERMARK`; `{"key": K, "id": I}` in its place makes the mark carry a trace id from 0 to 2^30 - 1, `{"id": I}` alone with the manager's key; `/v1/audio/watermark/detect` scores a recording against keys and with `"ids": true` reads the ids back; `/v1/audio/watermark/scan` finds the marked stretches of a long or spliced recording, each with its place and id), and `response_format` ("wav", or "pcm" for the headerless samples / code bytes
    as `audio/pcm`); streamed or not, the body's samples are the same bytes.  `encoding: "flac"` is its own container: the body is the
    native FLAC stream as `audio/flac` with a `.flac` file name, and `response_format` must be absent (400 with "wav" or "pcm" beside it);
    streamed, the stream header comes with the totals unknown."""
    from fastapi import APIRouter, FastAPI, HTTPException
    from starlette.responses import StreamingResponse

    models = request_models()

    def _options(req, allowed):
        """The request's sampler fields, checked (400) before anything is queued."""
        try:
            return tts_manager.request_options(allowed, **{k: getattr(req, k) for k in allowed})
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))

    def _response_format(req, opts):
        try:
            return container_format(req.response_format, opts.get("encoding"))
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))

    def _blocks(buf, size=1 << 16):
        """The body in 64 KiB blocks.  (Iterating the BytesIO itself yields "lines": a body is cut at every 0x0A byte, which G.711 code bytes
        are full of, and every piece costs a hop through the thread pool.)"""
        while True:
            block = buf.read(size)
            if not block:
                return
            yield block

    def _headers(filename, fmt):
        return {"Content-Disposition": f"attachment; filename={filename if fmt == 'wav' else filename.rsplit('.', 1)[0] + '.' + fmt}"}

    router = APIRouter(prefix="/v1", tags=["speech"])

    def _speech_options(text, req):
        """What both speech routes check first: a loaded model (503), the sampler fields and a non-empty text (400)."""
        if not tts_manager.model:
            raise HTTPException(status_code=503, detail="TTS model not loaded")
        opts = _options(req, infer.REQUEST_OPTIONS)
        if req.stream and stream_refusal(opts):
            raise HTTPException(status_code=400, detail=stream_refusal(opts))
        if not text.strip():
            raise HTTPException(status_code=400, detail="Text to synthesize cannot be empty.")
        return opts

    def _run(text, name, ref_text, filename, req):
        opts = _speech_options(text, req)
        fmt = _response_format(req, opts)
        try:
            buf = synthesize_speech(tts_manager, registry, text=text, ref_audio_name=name, ref_text=ref_text, response_format=fmt, **opts)
        except HTTPError as e:
            raise HTTPException(status_code=e.status_code, detail=e.detail)
        return StreamingResponse(_blocks(buf), media_type=MEDIA_TYPES[fmt], headers=_headers(filename, fmt))

    def _run_stream(text, name, ref_text, filename, req):
        """stream=true: the same checks as `_run`, then the first piece is synthesized BEFORE the response exists, so a bad request, an
        unloaded model or a failing first chunk still comes back as a status code.  The body is a streaming WAV (`wav_stream_header`)
        followed by the pieces in the delivery format (int16 PCM, or G.711 code bytes; no header with response_format "pcm").  With
        encoding "flac" the body is the FLAC stream alone (`audio/flac`): its 42-byte header with the totals unknown, which the manager's
        stream hands out only once the first chunk is there, then the frames as they complete.  A failure after the first bytes can only
        end the body early, and is logged."""
        opts = _speech_options(text, req)
        fmt = _response_format(req, opts)
        try:
            pieces = stream_speech(tts_manager, registry, text=text, ref_audio_name=name, ref_text=ref_text, **opts)
            first = next(pieces, None)
        except HTTPError as e:
            raise HTTPException(status_code=e.status_code, detail=e.detail)
        return StreamingResponse(_pcm_body(first, pieces, opts, fmt), media_type=MEDIA_TYPES[fmt], headers=_headers(filename, fmt))

    async def _pcm_body(first, pieces, opts, fmt):
        # the synthesis runs in the thread pool, one piece at a time; leaving early (client gone, error) closes the generator,
        # which cancels the request's remaining chunks if their batch has not started
        try:
            rate, enc = infer.WaveSpec.of(opts).format
            if fmt == "wav":
                yield wav_stream_header(rate, enc)
            if first is not None:
                yield delivery_bytes(first, enc)
            while True:
                piece = await run_in_threadpool(next, pieces, None)
                if piece is None:
                    break
                yield delivery_bytes(piece, enc)
        except Exception:   # noqa: BLE001 -- the status line is gone: end the body early
            log.exception("streamed synthesis failed after the first bytes; the response body ends early")
        finally:
            pieces.close()

    def _run_clone(req):
        """`/v1/audio/speech/clone`: the speech routes' checks, then the clip's (`TTSManager._clip_voice`: 400 with its message), then
        `synthesize_clip` -- or, with stream=true, `synthesize_clip_stream` with the first piece synthesized before the response exists."""
        opts = _speech_options(req.text, req)
        fmt = _response_format(req, opts)
        try:
            raw = base64.b64decode(req.ref_audio, validate=True)
        except (binascii.Error, ValueError):
            raise HTTPException(status_code=400, detail="Audio must be a base64-encoded WAV file.")
        headers = _headers("synthesized_speech.wav", fmt)
        try:
            if req.stream:
                pieces = tts_manager.synthesize_clip_stream(req.text, raw, req.ref_text, clip_short=req.clip_short, denoise=req.denoise, **opts)
                first = next(pieces, None)
                return StreamingResponse(_pcm_body(first, pieces, opts, fmt), media_type=MEDIA_TYPES[fmt], headers=headers)
            wave = tts_manager.synthesize_clip(req.text, raw, req.ref_text, clip_short=req.clip_short, denoise=req.denoise, **opts)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        return StreamingResponse(_blocks(response_body(wave, opts, fmt)), media_type=MEDIA_TYPES[fmt], headers=headers)

    def _run_script(req):
        """`/v1/audio/speech/script`: the speech routes' checks, each voice's (a registered name as on `/voice`, a clip as on `/clone`),
        then `synthesize_script` -- or, with stream=true, `synthesize_script_stream` with the first piece synthesized before the response."""
        opts = _speech_options(req.text, req)
        fmt = _response_format(req, opts)
        voices = {}
        for tag, v in req.voices.items():
            spec = dict(ref_text=v.ref_text, speed=v.speed)
            if (v.ref_audio_name is None) == (v.ref_audio is None):
                raise HTTPException(status_code=400, detail=f"Voice {tag!r} needs either ref_audio_name or ref_audio.")
            if v.ref_audio_name is not None:
                voice = registry.get(v.ref_audio_name)
                if voice is None:
                    raise HTTPException(status_code=400, detail="Invalid reference audio name.")
                spec.update(ref_audio_path=voice.audio_path, ref_text=v.ref_text or voice.ref_text)
            else:
                try:
                    spec.update(ref_audio=base64.b64decode(v.ref_audio, validate=True), clip_short=v.clip_short)
                except (binascii.Error, ValueError):
                    raise HTTPException(status_code=400, detail="Audio must be a base64-encoded WAV file.")
            if not spec["ref_text"] or not spec["ref_text"].strip():
                raise HTTPException(status_code=400, detail="Reference text cannot be empty.")
            if "denoise" in (v.model_extra or {}):   # checked by the manager: true or false, and of an uploaded clip only
                spec.update(denoise=v.model_extra["denoise"])
            voices[tag] = spec
        headers = _headers("synthesized_script.wav", fmt)
        try:
            if req.stream:
                pieces = tts_manager.synthesize_script_stream(req.text, voices, gap=req.gap, **opts)
                first = next(pieces, None)
                return StreamingResponse(_pcm_body(first, pieces, opts, fmt), media_type=MEDIA_TYPES[fmt], headers=headers)
            wave = tts_manager.synthesize_script(req.text, voices, gap=req.gap, **opts)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        return StreamingResponse(_blocks(response_body(wave, opts, fmt)), media_type=MEDIA_TYPES[fmt], headers=headers)

    def _run_edit(req):
        if not tts_manager.model:
            raise HTTPException(status_code=503, detail="TTS model not loaded")
        opts = _options(req, tuple(dict.fromkeys(EDIT_OPTIONS + EDIT_DELIVERY + EDIT_MARK)))
        if req.denoise is not None:
            raise HTTPException(status_code=400, detail="denoise is an option of an uploaded reference clip: the edit route keeps the recording")
        fmt = _response_format(req, opts)
        try:
            raw = base64.b64decode(req.audio, validate=True)
        except (binascii.Error, ValueError):
            raise HTTPException(status_code=400, detail="Audio must be a base64-encoded WAV file.")
        if not req.text.strip():
            raise HTTPException(status_code=400, detail="Text to synthesize cannot be empty.")
        try:
            audio = tts_manager.decode_audio(raw)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=f"Invalid audio: {e}")
        try:
            wave = tts_manager.edit(audio, req.text, req.parts_to_edit, req.fix_duration, **opts)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        return StreamingResponse(_blocks(response_body(wave, opts, fmt)), media_type=MEDIA_TYPES[fmt], headers=_headers("edited_speech.wav", fmt))

    def _run_detect(req):
        """`/v1/audio/watermark/detect`: {"audio": base64 WAV or FLAC, "keys"?: [1 .. 16 keys]} -> {"results": [{"key", "detected", "score",
        "offset"}]}, one per key (`TTSManager.detect_watermark`; no key in the body: the manager's own).  Needs no loaded model.  With "ids": true
        each result also has "id" (the trace id the key's mark carries, or null) and "id_score" (`TTSManager.read_watermark`)."""
        try:
            raw = base64.b64decode(req.audio, validate=True)
        except (binascii.Error, ValueError):
            raise HTTPException(status_code=400, detail="Audio must be a base64-encoded WAV or FLAC file.")
        try:
            keys = None if req.keys is None else infer.check_watermark_keys(req.keys)   # (before the recording is decoded)
            if req.ids is not None and not isinstance(req.ids, bool):
                raise ValueError(f"ids must be true or false (got {req.ids!r})")
            try:
                audio = tts_manager.decode_audio(raw)
            except ValueError as e:
                raise ValueError(f"Invalid audio: {e}") from e
            scores = tts_manager.read_watermark(audio, keys) if req.ids else tts_manager.detect_watermark(audio, keys)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        if req.ids:
            return {"results": [dict(key=s.key, detected=s.detected, score=s.z, offset=s.offset, id=s.id, id_score=s.id_z) for s in scores]}
        return {"results": [dict(key=s.key, detected=s.detected, score=s.z, offset=s.offset) for s in scores]}

    def _run_scan(req):
        """`/v1/audio/watermark/scan`: {"audio": base64 WAV or FLAC, "keys"?: [1 .. 16 keys]} -> {"seconds", "spans": [{"key", "start", "end",
        "score", "offset", "id", "id_score"}]}: the marked stretches of a long or spliced recording (`TTSManager.scan_watermark`; no key in the
        body: the manager's own), start and end in seconds of the recording at 24 kHz, "id" the stretch's trace id or null.  Needs no loaded
        model.  400 for bad keys, no key anywhere, audio that cannot be read and a recording over 600 s."""
        try:
            raw = base64.b64decode(req.audio, validate=True)
        except (binascii.Error, ValueError):
            raise HTTPException(status_code=400, detail="Audio must be a base64-encoded WAV or FLAC file.")
        try:
            keys = None if req.keys is None else infer.check_watermark_keys(req.keys)   # (before the recording is decoded)
            try:
                wave, sr = tts_manager.decode_audio(raw)
            except ValueError as e:
                raise ValueError(f"Invalid audio: {e}") from e
            spans = tts_manager.scan_watermark((wave, sr), keys)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        rate = float(infer.target_sample_rate)
        return {"seconds": wave.shape[-1] / float(sr),
                "spans": [dict(key=s.key, start=s.start / rate, end=s.end / rate, score=s.z, offset=s.offset, id=s.id, id_score=s.id_z) for s in spans]}

    def _run_check(req):
        """`/v1/audio/reference/check`: {"audio": base64 WAV or FLAC, "clip_short"?: true} -> {"report": {seconds, rms, peak, clipped, clip_ratio,
        noise_db, snr_db, speech_ratio, bandwidth_hz}, "problems": [...]}: the clip's measures (`TTSManager.check_reference`; an infinite
        noise_db / snr_db is null) and the manager's limits it violates (none without limits).  A bad upload is the clone route's 400."""
        try:
            raw = base64.b64decode(req.audio, validate=True)
        except (binascii.Error, ValueError):
            raise HTTPException(status_code=400, detail="Audio must be a base64-encoded WAV file.")
        try:
            report = tts_manager.check_reference(raw, req.clip_short)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        return {"report": report.as_json(), "problems": tts_manager.reference_problems(report)}

    # The reference's handlers are `async def` around a blocking call, i.e. one request at a time.  Here the blocking part runs in
    # starlette's thread pool, so concurrent requests overlap and meet in the MicroBatcher queue (when the manager has one).
    from starlette.concurrency import run_in_threadpool

    @router.post("/audio/speech", response_class=StreamingResponse)
    async def synthesize_kannada(request: models.KannadaSynthesizeRequest):
        return await run_in_threadpool(_run_stream if request.stream else _run, request.text, registry.default_voice, None,
                                       "synthesized_kannada_speech.wav", request)

    @router.post("/audio/speech/voice", response_class=StreamingResponse)
    async def synthesize_with_voice(request: models.SynthesizeRequest):     # the generic form the reference's helper already supports
        return await run_in_threadpool(_run_stream if request.stream else _run, request.text, request.ref_audio_name, request.ref_text,
                                       "synthesized_speech.wav", request)

    @router.post("/audio/speech/clone", response_class=StreamingResponse)
    async def synthesize_with_clip(request: models.CloneRequest):          # the caller's own reference clip (TTSManager.synthesize_clip)
        return await run_in_threadpool(_run_clone, request)

    @router.post("/audio/speech/script", response_class=StreamingResponse)
    async def synthesize_script(request: models.ScriptRequest):            # a multi-voice `[tag]` script as one request (TTSManager.synthesize_script)
        return await run_in_threadpool(_run_script, request)

    @router.post("/audio/edit", response_class=StreamingResponse)
    async def edit_speech(request: models.EditRequest):                    # speech editing (F/infer/speech_edit.py) over the same manager
        return await run_in_threadpool(_run_edit, request)

    @router.post("/audio/watermark/detect")
    async def detect_watermark(request: models.DetectRequest):            # provenance: does this recording carry a key's mark?
        return await run_in_threadpool(_run_detect, request)

    @router.post("/audio/watermark/scan")
    async def scan_watermark(request: models.ScanRequest):                # provenance: where in this recording are the marked stretches, and whose?
        return await run_in_threadpool(_run_scan, request)

    @router.post("/audio/reference/check")
    async def check_reference(request: models.ReferenceCheckRequest):      # is this clip fit to clone from?
        return await run_in_threadpool(_run_check, request)

    app = FastAPI(title="F5-TTS on MI355X (HIP path)")
    app.include_router(router)
    return app


# ---------------------------------------------------------------------------------------------------------------- multi-GPU backend
class ShardedJobError(RuntimeError):
    """A rank of a sharded job failed.  Every rank still took part in the job's collectives (so nobody hangs), but the job has no
    result and the batch must not be retried request by request on a backend in an unknown state: `no_retry` tells MicroBatcher so, the
    sampler refuses further jobs, and the serving process should exit non-zero so that its supervisor starts fresh ranks."""
    no_retry = True


class ShardedSampler:
    """The model object of rank 0 in a one-process-per-GPU serving job: `sample_units` deals the units of a batch over the ranks
    (`sharding.shard_units`: longest-processing-time dealing with the SURVEY 8(d) cost model), every rank -- this one included --
    samples its share on its own GPU with its own replica of the weights, and the mels come back to rank 0 in unit order.
    There is no collective inside the ODE loop: one job broadcast (tokens, frame counts, the reference mels of the voices in the
    batch: 188 KB per voice) and one gather per batch, RCCL over xGMI when the process group's backend is "nccl".
    Ranks > 0 run `rank_worker_loop(local_model)`; `close()` on rank 0 releases them.
    Failure: a rank whose local `sample_units` raises still joins the gather with a failure header; rank 0 then raises
    `ShardedJobError` after the collective has completed on every rank, and refuses later jobs (`failed`).
    Noise: every rank draws the noise of ITS units from its own generator (like the reference's per-call `torch.randn`, unseeded in
    `infer_batch_process`), so an unseeded result is not reproducible across world sizes; pass `seed=` in the knobs for that.  Units with
    their own generator (`generators=`, a seeded request's chunks) get their noise drawn HERE, on rank 0, in unit order at the unit's final
    duration (`model.unit_duration`), and broadcast with the job: a seeded unit gets the same noise whichever rank samples it.
    Per-unit `cfg_strength`, `steps`, `sway_sampling_coef` and `ode_method` (lists) are sliced to each rank's units (one `ode_method` name
    for all units rides in the job's knobs as it is); the sampler declares
    `per_unit_time_grids` when its local model does, so `infer.infer_requests` hands it units of different time grids in one call.  (Ranks > 0 do not switch their handles to the shape-invariant
    attention mode yet, so the bit-for-bit promises of a seeded request hold on one GPU.)
    Streaming (`TTSManager.synthesize_stream`) needs nothing here: a stream's first chunk and its remaining chunks arrive as units of
    ordinary `sample_units` batches."""

    def __init__(self, local_model, device=None):
        import torch
        import torch.distributed as dist
        self.local, self.dist, self.torch = local_model, dist, torch
        self.device = device if device is not None else getattr(local_model, "device", torch.device("cpu"))
        self.vocab_char_map = getattr(local_model, "vocab_char_map", None)
        self.failed: str | None = None

    @property
    def per_unit_time_grids(self):
        return bool(getattr(self.local, "per_unit_time_grids", False))

    # what infer.* needs from a model object
    def cond_mel(self, audio):
        return self.local.cond_mel(audio)

    def prepare_voices(self, voices):
        if hasattr(self.local, "prepare_voices"):
            return self.local.prepare_voices(voices)
        return infer.prepare_voices(voices, device=None)

    def sample_units(self, audio, units, **knobs):
        if self.failed:
            raise ShardedJobError(f"sharded backend is down: {self.failed}")
        from .model import per_unit_cfg, per_unit_values, unit_duration
        torch = self.torch
        b = len(units)
        audios = list(audio) if isinstance(audio, (list, tuple)) else [audio] * b
        voices, voice_of = [], []
        for a in audios:                                   # distinct voices of the batch, by object identity
            for k, v in enumerate(voices):
                if v is a:
                    voice_of.append(k)
                    break
            else:
                voices.append(a)
                voice_of.append(len(voices) - 1)
        mels = [(self.local.cond_mel(a) if a.ndim == 2 else a)[0].to(torch.float32) for a in voices]
        knobs = dict(knobs)
        gens, y0 = knobs.pop("generators", None), knobs.pop("y0", None)
        cfg, per_unit = knobs.get("cfg_strength"), None
        if cfg is not None and per_unit_cfg(cfg, b) is not None:
            per_unit, knobs["cfg_strength"] = [float(c) for c in cfg], None      # replaced per rank by its units' slice
        grids = {}                            # per-unit time grids: sliced per rank like the strengths
        for name in ("steps", "sway_sampling_coef"):
            v = per_unit_values(knobs.get(name), b, name)
            if isinstance(v, list):
                grids[name] = [None if x is None else (int(x) if name == "steps" else float(x)) for x in v]
                knobs[name] = None
        if isinstance(knobs.get("ode_method"), (list, tuple)):   # per-unit solvers: sliced per rank too
            grids["ode_method"] = list(knobs.pop("ode_method"))
            if len(grids["ode_method"]) != b:
                raise ValueError(f"ode_method: one name per unit ({b}) or one name, got {len(grids['ode_method'])} values")
        noise = list(y0) if y0 is not None else [None] * b
        if gens is not None:
            mel_dim = mels[0].shape[1]
            for i, ((tokens, frames), g) in enumerate(zip(units, gens)):
                if g is not None and noise[i] is None:
                    dur = unit_duration(mels[voice_of[i]].shape[0], len(tokens), frames)
                    noise[i] = torch.randn(dur, mel_dim, generator=g)
        noise_rows = [0 if n is None else int(n.shape[0]) for n in noise]
        job = dict(units=[(list(t), int(f)) for t, f in units], voice_of=voice_of, mel_shapes=[tuple(m.shape) for m in mels], knobs=knobs,
                   cfg=per_unit, noise_rows=noise_rows)
        if grids:
            job["grids"] = grids
        try:
            return _run_sharded_job(self.local, job, mels, self.device, noise if any(noise_rows) else None)
        except ShardedJobError as e:
            self.failed = str(e)
            raise

    def close(self):
        if self.dist.is_initialized() and self.dist.get_world_size() > 1:
            self.dist.broadcast_object_list([None], src=0)


def _run_sharded_job(local_model, job, mels, device, noise=None):
    """Collective part shared by rank 0 (`job`, `mels` given) and the workers (both None): returns the mels of all units on rank 0.
    Every rank that entered the job's broadcast also enters its gather, whatever its local sampler did.  `noise` (rank 0): per unit the
    [dur, mel] noise drawn from its own generator, or None; broadcast in one payload when any unit has one (`job["noise_rows"]`)."""
    import sys
    import traceback

    import torch
    import torch.distributed as dist
    from .sharding import gather_waves, shard_units
    multi = dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if multi else (0, 1)
    if multi:
        box = [job]
        dist.broadcast_object_list(box, src=0)
        job = box[0]
        if job is None:
            return None
        flat = torch.cat([m.reshape(-1) for m in mels]).to(device) if rank == 0 else torch.empty(sum(a * b for a, b in job["mel_shapes"]), device=device)
        dist.broadcast(flat, src=0)
        mels, k = [], 0
        for a, b in job["mel_shapes"]:
            mels.append(flat[k:k + a * b].view(a, b))
            k += a * b
        rows, mel_dim = job.get("noise_rows") or [], job["mel_shapes"][0][1]
        if any(rows):   # the seeded units' noise, drawn on rank 0
            if rank == 0:
                buf = torch.cat([n.reshape(-1).to(device, torch.float32) for n in noise if n is not None])
            else:
                buf = torch.empty(sum(rows) * mel_dim, dtype=torch.float32, device=device)
            dist.broadcast(buf, src=0)
            noise, k = [], 0
            for r in rows:
                noise.append(buf[k:k + r * mel_dim].view(r, mel_dim) if r else None)
                k += r * mel_dim
    units = job["units"]
    shards = shard_units([f for _, f in units], world)
    mine = shards[rank]
    # payload of a rank: a status word (number of units, or -1: the local sampler failed), the row count of each unit, then their rows
    # (a unit's final duration can exceed the planned frames: sample() raises it to lens + 1 like the reference, cfm.py:136)
    local_error = None
    knobs = dict(job["knobs"])
    if job.get("cfg") is not None:        # per-unit CFG strengths: this rank's units
        knobs["cfg_strength"] = [job["cfg"][i] for i in mine]
    for name, vals in (job.get("grids") or {}).items():   # per-unit steps / sway / solver: this rank's units
        knobs[name] = [vals[i] for i in mine]
    if noise is not None and any(noise[i] is not None for i in mine):
        knobs["y0"] = [noise[i] for i in mine]
    try:
        outs = local_model.sample_units([mels[job["voice_of"][i]][None] for i in mine], [units[i] for i in mine], **knobs) if mine else []
        if len(outs) != len(mine):
            raise RuntimeError(f"sample_units returned {len(outs)} mels for {len(mine)} units")
        head = torch.tensor([float(len(outs))] + [float(o.shape[0]) for o in outs], dtype=torch.float32, device=device)
        packed = torch.cat([head] + [o.reshape(-1).to(device, torch.float32) for o in outs])
    except Exception as e:   # noqa: BLE001 -- reported through the collective, never by leaving it
        local_error = e
        traceback.print_exc(file=sys.stderr)
        packed = torch.tensor([-1.0], dtype=torch.float32, device=device)
    got = gather_waves(packed, dst=0)
    if rank != 0:
        return []
    bad = [r for r, flat_r in enumerate(got) if float(flat_r[0]) < 0]
    if bad:
        err = ShardedJobError(f"sample_units failed on rank(s) {bad} of {world}" + (f": {local_error!r}" if local_error is not None else ""))
        raise err from local_error
    mel_dim = mels[0].shape[1]
    result = [None] * len(units)
    for r, flat_r in enumerate(got):
        k = 1 + len(shards[r])
        for j, i in enumerate(shards[r]):
            n = int(flat_r[1 + j])
            result[i] = flat_r[k:k + n * mel_dim].view(n, mel_dim)
            k += n * mel_dim
    return result


def rank_worker_loop(local_model, device=None):
    """What ranks > 0 of a serving job run: take part in every job rank 0's `ShardedSampler` broadcasts until it closes.  A job whose
    local sampler raised is reported to rank 0 inside the job's gather (`_run_sharded_job`) and the loop goes on."""
    import torch
    device = device if device is not None else getattr(local_model, "device", torch.device("cpu"))
    n = 0
    while _run_sharded_job(local_model, None, None, device) is not None:
        n += 1
    return n
