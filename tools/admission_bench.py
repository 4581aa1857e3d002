#!/usr/bin/env python3
"""Admission latency of the serving queue: one fixed, seeded arrival trace replayed through `serve.MicroBatcher` (a request waits for the
batch in front of it to end) and through `serve.ContinuousBatcher` (it joins the running batch at the next span boundary), on the same
model objects in one process.

    python tools/admission_bench.py [--requests 48] [--load 0.7] [--spans 4 8 16 32] [--seed 0]

Workload: F5-TTS Base width (synthetic weights), 32 NFE, CFG 2, sway -1, Vocos, shape-invariant attention as served; a 5 s prompt and a
one-chunk text of about 10 s (~1 450 frames per request).  First the capacity of the MicroBatcher path is measured (16 requests submitted
at once, requests / s); the trace is Poisson arrivals at `--load` times that rate, every fourth request streamed
(`TTSManager.synthesize_stream`).  Per run: submit -> admission (the `on_start` hook of both batchers: the request's batch has formed /
the request was planned into the running batch), submit -> result, submit -> first audio of the streamed requests, generated mel frames
per second over the run's makespan.  The MicroBatcher runs twice: the spread of the yardstick.  Then the fixed cost of a span: wall clock
of one `advance` call (device sync) over 1 and 2 steps for 1 and 8 units, fixed = 2 T(1) - T(2), split with the library's per-class
HIP-event times (f5hip_dit_get_profile) into the text / conditioning / time precompute on the device and the rest (sequence set-up,
uploads, the state copies), in ms and as a share of a span of each length.
Wall clock on the host, after a warm-up of both paths."""
import argparse
import os
import statistics
import sys
import tempfile
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import infer, serve, synth  # noqa: E402
from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel  # noqa: E402
from tts_indic_server_f5_amd.vocoder import F5HipVocos  # noqa: E402
from tools.stream_latency import REF_TEXT, TEXT, VOCAB, _prompt_wav  # noqa: E402

SENTENCE = TEXT.split(". ")[0] + "."      # one chunk


def replay(mgr, path, arrivals, seed0):
    """Replays the trace; per request (admission, result, first audio or None), seconds after its submit, and the makespan."""
    voice, ref_text = mgr._voice(path, REF_TEXT)
    out, t_start = [None] * len(arrivals), time.perf_counter()

    def client(i, at):
        time.sleep(max(0.0, t_start + at - time.perf_counter()))
        t0, mark = time.perf_counter(), {}
        if i % 4 == 3:
            first = None
            for _ in mgr.synthesize_stream(SENTENCE, ref_audio_path=path, ref_text=REF_TEXT, seed=seed0 + i):
                first = first if first is not None else time.perf_counter() - t0
            out[i] = (None, time.perf_counter() - t0, first)
        else:
            req = mgr._request(voice, ref_text, SENTENCE, dict(seed=seed0 + i))
            mgr.batcher.submit(req, on_start=lambda: mark.setdefault("t", time.perf_counter() - t0)).result(timeout=600)
            out[i] = (mark.get("t"), time.perf_counter() - t0, None)

    threads = [threading.Thread(target=client, args=(i, at)) for i, at in enumerate(arrivals)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return out, time.perf_counter() - t_start


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def report(name, rows, makespan, frames):
    adm = [r[0] for r in rows if r[0] is not None]
    res = [r[1] for r in rows]
    ttfa = [r[2] for r in rows if r[2] is not None]
    print(f"{name:>22} | admission p50 {statistics.median(adm) * 1e3:8.1f} p95 {pct(adm, 0.95) * 1e3:8.1f} ms | result p50 {statistics.median(res) * 1e3:8.1f} "
          f"p95 {pct(res, 0.95) * 1e3:8.1f} ms | first audio (streamed) p50 {statistics.median(ttfa) * 1e3:8.1f} p95 {pct(ttfa, 0.95) * 1e3:8.1f} ms | "
          f"{frames * len(rows) / makespan:9.0f} mel-frames/s", flush=True)
    return statistics.median(adm), frames * len(rows) / makespan


def span_fixed_cost(model, voice, tokens, frames, reps=5):
    """T(k), the wall clock of one `advance` of k steps (device sync; profiling off), and D_c(k), the library's HIP-event time of kernel
    class c in such a call (totals reset before each call, read after it).  A step costs T(2) - T(1); what a span pays once is
    2 T(1) - T(2).  Of that, 2 D_c(1) - D_c(2) is device time of the profiled launches outside the step loop: the text, conditioning
    and time precompute.  The rest is host work and copies: sequence set-up, the uploads of the tables, the state cat / copy_."""
    def timed(n_units, k, profile):
        ts, ds = [], []
        for _ in range(reps + 1):
            units = [model.plan_unit(voice, tokens, frames, steps=32, generator=torch.Generator().manual_seed(i)) for i in range(n_units)]
            torch.cuda.synchronize()
            if profile:
                model.set_profiling(True)           # (also resets the totals)
            t0 = time.perf_counter()
            model.advance(units, k)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            if profile:
                ds.append({c: v["total_ms"] for c, v in model.get_profile().items()})
                model.set_profiling(False)
        return statistics.median(ts[1:]) * 1e3, {c: statistics.median(d[c] for d in ds[1:]) for c in (ds[0] if ds else ())}

    for n_units in (1, 8):
        (t1, _), (t2, _) = timed(n_units, 1, False), timed(n_units, 2, False)
        (_, d1), (_, d2) = timed(n_units, 1, True), timed(n_units, 2, True)
        fixed, step = 2 * t1 - t2, t2 - t1
        dev = {c: 2 * d1[c] - d2[c] for c in d1}
        pre = sum(dev.values())
        print(f"span of {n_units} unit(s): 1 step {t1:.2f} ms, 2 steps {t2:.2f} ms -> one step {step:.2f} ms, fixed cost {fixed:.2f} ms per span = "
              + ", ".join(f"{fixed / (fixed + k * step) * 100:.1f} % of a {k}-step span" for k in (4, 8, 16, 32)), flush=True)
        print(f"    of the fixed cost: text / cond / time precompute on the device {pre:.2f} ms (" + ", ".join(f"{c} {v:.2f}" for c, v in dev.items())
              + f"; per step: " + ", ".join(f"{c} {d2[c] - d1[c]:.2f}" for c in d1) + f"); sequence set-up, uploads and state copies {fixed - pre:.2f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=48)
    ap.add_argument("--load", type=float, default=0.7)
    ap.add_argument("--spans", type=int, nargs="+", default=[4, 8, 16, 32])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    model = F5HipModel(F5TTS_BASE, synth.dit_state_dict(), vocab_char_map=VOCAB)
    voc = F5HipVocos(synth.vocos_state_dict())
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "prompt.wav")
        _prompt_wav(path)

        def manager(**micro_batch):
            return serve.TTSManager(nfe_step=32, micro_batch=micro_batch).load(model, voc)

        mgr = manager(max_requests=16, max_wait_ms=5)
        voice, ref_text = mgr._voice(path, REF_TEXT)
        wave = mgr.synthesize(SENTENCE, ref_audio_path=path, ref_text=REF_TEXT, seed=1)
        frames = len(wave) // 256 + 1
        replay(mgr, path, [0.0] * 16, 1000)                                            # warm-up at the largest batch
        _, t16 = replay(mgr, path, [0.0] * 16, 2000)
        capacity = 16 / t16
        rate = args.load * capacity
        arrivals = np.cumsum(np.random.default_rng(args.seed).exponential(1.0 / rate, args.requests)).tolist()
        print(f"workload: F5-TTS Base, 32 NFE, CFG 2, sway -1, Vocos; one chunk of {frames} generated frames per request; device {torch.cuda.get_device_name(0)}")
        print(f"MicroBatcher capacity (16 requests at once): {capacity:.2f} requests/s; trace: {args.requests} Poisson arrivals at {rate:.2f} requests/s "
              f"({args.load:.0%}), seed {args.seed}, over {arrivals[-1]:.2f} s; every fourth request streamed")
        base = [report(f"MicroBatcher run {k + 1}", *replay(mgr, path, arrivals, 3000), frames) for k in range(2)]
        mgr.batcher.close()
        results = {}
        for s in args.spans:
            cmgr = manager(span_steps=s, max_frames=16 * 2048)
            replay(cmgr, path, [0.0] * 4, 1000)                                        # warm-up of the span path
            results[s] = report(f"ContinuousBatcher s={s}", *replay(cmgr, path, arrivals, 3000), frames)
            cmgr.batcher.close()
        spread = abs(base[0][1] - base[1][1]) / max(base[0][1], base[1][1])
        print(f"MicroBatcher run-to-run spread of mel-frames/s: {spread:.1%}")
        for s, (adm, fps) in results.items():
            print(f"span_steps {s:>2}: median admission {adm * 1e3:.1f} ms vs {min(b[0] for b in base) * 1e3:.1f} ms; mel-frames/s {fps / max(b[1] for b in base) - 1:+.1%} vs the better MicroBatcher run")
        _, ((tokens, unit_frames),) = infer._plan_request(voice, ref_text, [SENTENCE], infer.target_rms, 1.0, None, None, infer.text_to_tokens)
        span_fixed_cost(model, voice.cond(model), tokens, unit_frames)


if __name__ == "__main__":
    main()
