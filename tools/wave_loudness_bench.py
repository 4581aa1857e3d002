#!/usr/bin/env python3
"""What a per-request loudness target costs: from a micro-batch's vocoded chunks to every request's finished PCM on the host.

    python tools/wave_loudness_bench.py [--reps 15] [--out profiles/wave_loudness_bench.txt] [--parent TREE] [--kernel-db DB]

The clock starts when the vocoder returns -- a stand-in `decode_ragged` hands out views of one packed fp32 buffer that is already on the
device, as F5HipVocos does -- and stops when every request's PCM is on the host.  Tails, alternating in one process:
     host+loudness    `finish_requests(device_backend=False, loudness=-16)`: the chunk waves come down, then join, quantisation and
                      `normalise_loudness_pcm16` in numpy
     device           `finish_requests(device_backend=True)` without the option: ONE f5hip_wave_finish call, one download
     device+loudness  the same with `loudness=-16`: ONE f5hip_wave_loudness call (three launches) behind wave_finish, in place
Batches: 8 requests of one chunk of about 10 s, and a ragged one (0.3 s to 17 s).  Wall clock with a device sync, median and min..max of
`--reps` (at least 7) after a warm-up round.  Then the library call alone, `ops.wave_loudness` on PCM that is already on the device, in HIP
events (median of `--reps` after a warm-up) next to `normalise_loudness_pcm16` of the same PCM on the host; and launch 1's share of it by
difference: the same call on silent PCM (nothing passes the gates: launch 3 returns at once) minus the same call with every device length 0
(all three launches return at once), as MACs per second: samples x 1024 taps over that time.  (The kernel skips nothing for silence: the time
of its FMAs does not depend on the data.)

`--parent TREE`: a checkout of the parent commit, built; the "device" tail without the option is timed for the same batches in child
processes that run nothing else: the parent's tree, this tree, the parent's again (the spread between the two parent runs is the noise).
`--kernel-db DB`: the rocpd database of a `rocprofv3 --kernel-trace` run of `--trace-loop N` (N device calls on the 8 x 10 s batch and
nothing else): the three kernels' own times.  `--tree TREE`: import the package from TREE (what the child process is given).

Nothing is decided by this file: `serve.DEVICE_BACKEND_DEFAULT` stays as it is, and no threshold is set."""
import argparse
import json
import os
import sqlite3
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_args = argparse.ArgumentParser()
_args.add_argument("--reps", type=int, default=15)
_args.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_loudness_bench.txt"))
_args.add_argument("--parent", default=None)
_args.add_argument("--kernel-db", default=None)
_args.add_argument("--trace-loop", type=int, default=0)
_args.add_argument("--tree", default=ROOT)
_args.add_argument("--plain-only", action="store_true", help="time the `device` tail alone and print one JSON line (the --parent child)")
ARGS = _args.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import infer  # noqa: E402

RATE, HOP, TAPS = 24000, 256, 1024
TARGET = -16.0
BATCHES = {"8 x 10 s": [938] * 8, "ragged, 8 requests of 0.3 .. 17 s": [30, 1600, 470, 938, 95, 1220, 700, 260]}   # vocoder frames per request


def _speech_like(n, seed, amp=0.12):
    g = np.random.default_rng(seed)
    t = np.arange(n) / float(RATE)
    w = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(g.uniform(80, 4000, 8), g.uniform(0, 2 * np.pi, 8))) / np.sqrt(8)
    env = 0.6 + 0.4 * np.sin(2 * np.pi * 2.7 * t + seed)
    return (amp * env * w + 0.01 * g.standard_normal(n)).astype(np.float32)


class PackedVocoder:
    """`decode_ragged` as F5HipVocos answers it: views of one packed device buffer, which is made before the clock starts"""

    def __init__(self, frames, device):
        self.lens = [(f - 1) * HOP for f in frames]
        self.packed = torch.from_numpy(np.concatenate([_speech_like(n, 7 + i, 0.03 + 0.04 * i) for i, n in enumerate(self.lens)])).to(device)

    def decode_ragged(self, mels):
        return list(self.packed.split(self.lens))


def _fmt(ts, unit=1e3):
    return f"{statistics.median(ts) * unit:9.3f} ms  ({min(ts) * unit:.3f} .. {max(ts) * unit:.3f})"


def _tails(frames, device, loudness):
    voc = PackedVocoder(frames, device)
    groups = [([torch.zeros(f, 100, device=device)], 0, torch.tensor(0.2)) for f in frames]
    texts = ["x"] * len(frames)

    def run(backend, **kw):
        waves = [w for w, _ in infer._chunk_waves(groups, voc, "vocos", infer.target_rms, on_device=backend, want_specs=False)]
        return infer.finish_requests(waves, texts, infer.cross_fade_duration, device_backend=backend, want="pcm16", **kw)

    tails = [("device", lambda: run(True))]
    if loudness:
        tails = [("host+loudness", lambda: run(False, loudness=TARGET))] + tails + [("device+loudness", lambda: run(True, loudness=TARGET))]
    return voc, tails


def _time_tails(tails, reps):
    times, results, stats = {name: [] for name, _ in tails}, {}, {}
    for rep in range(reps + 1):                      # the first round warms everything up (workspaces, allocator, numpy buffers, the tap table)
        for name, fn in tails:
            infer.backend_stats.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
            stats[name] = dict(infer.backend_stats)
    return times, results, stats


def plain_only(reps, device):
    out = {}
    for what, frames in BATCHES.items():
        _, tails = _tails(frames, device, loudness=False)
        out[what] = _time_tails(tails, reps)[0]["device"]
    print("PLAIN " + json.dumps(out), flush=True)


def _events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return ts


def _counter(name):
    import ctypes as C
    from tts_indic_server_f5_amd import _lib
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _packed_pcm(frames, device, silent=False):
    lens = [(f - 1) * HOP for f in frames]
    offsets, off = [], 0
    for n in lens:
        offsets.append(off)
        off += (n + 7) & ~7
    buf = np.zeros(off, dtype=np.int16)
    pcms = [infer.quantise_pcm16(_speech_like(n, 7 + i, 0.03 + 0.04 * i)) for i, n in enumerate(lens)]
    if not silent:
        for o, x in zip(offsets, pcms):
            buf[o:o + len(x)] = x
    return torch.from_numpy(buf).to(device), offsets, lens, pcms


def library_call(what, frames, reps, device, emit):
    from tts_indic_server_f5_amd import _lib, ops
    pcm0, offsets, lens, pcms = _packed_pcm(frames, device)
    silent, _, _, _ = _packed_pcm(frames, device, silent=True)
    ks = [infer.loudness_gain_constant(TARGET)] * len(lens)
    zero_len = torch.zeros(len(lens), dtype=torch.int32, device=device)
    work = pcm0.clone()

    def call():                                       # (every call meets the same samples: the copy is queued in front of it, outside the events)
        ops.wave_loudness(work, offsets, lens, None, ks)

    ts = []
    for rep in range(reps + 1):
        work.copy_(pcm0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if rep:
            ts.append(a.elapsed_time(b) * 1e-3)
    same = all(np.array_equal(work[o:o + n].cpu().numpy(), infer.normalise_loudness_pcm16(x, TARGET)) for o, n, x in zip(offsets, lens, pcms))
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset")
    call()
    launches = _counter("wave_loudness_launches")
    host = []
    for rep in range(min(reps, 7) + 1):
        t0 = time.perf_counter()
        for x in pcms:
            infer.normalise_loudness_pcm16(x, TARGET)
        if rep:
            host.append(time.perf_counter() - t0)
    t_silent = _events(lambda: ops.wave_loudness(silent, offsets, lens, None, ks), reps)
    t_empty = _events(lambda: ops.wave_loudness(silent, offsets, lens, zero_len, ks), reps)
    fir = statistics.median(t_silent) - statistics.median(t_empty)
    macs = float(sum(lens)) * TAPS
    emit(f"  {what}: {sum(lens)} samples, {launches} launches per call (device result equals the host function's bytes: {same})")
    emit(f"      ops.wave_loudness, HIP events         {_fmt(ts)}")
    emit(f"      normalise_loudness_pcm16 on the host  {_fmt(host)}   ({statistics.median(host) / statistics.median(ts):.0f} x the device call)")
    emit(f"      the call on silent PCM                {_fmt(t_silent)}   with every device length 0: {_fmt(t_empty)}")
    emit(f"      launch 1 by difference: {fir * 1e3:.3f} ms for {macs / 1e9:.3f} G MACs = {macs / fir / 1e12:.2f} T MAC/s "
         f"({100 * macs / fir / 39.3e12:.1f} % of the 39.3 T fp64 FMA/s of the data sheet's 78.6 TFLOPS)")
    return macs


def kernel_db(path, macs, emit):
    rows = sqlite3.connect(path).execute("select name, duration from kernels").fetchall()
    emit(f"kernel times of a rocprofv3 --kernel-trace run of the 8 x 10 s call ({os.path.basename(path)}):")
    for key in ("wave_kweight_kernel", "wave_gate_kernel", "wave_gain_kernel"):
        d = sorted(d for name, d in rows if key in name)
        if not d:
            emit(f"  {key}: not in the trace")
            continue
        med = d[len(d) // 2] * 1e-9
        rate = f"   {macs / med / 1e12:.2f} T MAC/s, {100 * macs / med / 39.3e12:.1f} % of 39.3 T fp64 FMA/s" if key == "wave_kweight_kernel" else ""
        emit(f"  {key:20s} {len(d):4d} launches, median {med * 1e6:9.1f} us ({d[0] * 1e-3:.1f} .. {d[-1] * 1e-3:.1f}){rate}")


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    device = torch.device("cuda:0")
    reps = max(ARGS.reps, 7)
    if ARGS.plain_only:
        return plain_only(reps, device)
    if ARGS.trace_loop:
        from tts_indic_server_f5_amd import ops
        pcm0, offsets, lens, _ = _packed_pcm(BATCHES["8 x 10 s"], device)
        work = pcm0.clone()
        for _ in range(ARGS.trace_loop):
            work.copy_(pcm0)
            ops.wave_loudness(work, offsets, lens, None, [infer.loudness_gain_constant(TARGET)] * len(lens))
        torch.cuda.synchronize()
        return
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    emit(f"tools/wave_loudness_bench.py: median (min .. max) of {reps} after a warm-up round; target {TARGET} LUFS on every request")
    emit(f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")
    alone = {}
    for who, tree in (("parent commit", ARGS.parent), ("this commit", ROOT), ("parent commit, again", ARGS.parent)) if ARGS.parent else ():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--tree", tree, "--reps", str(reps)], capture_output=True, text=True,
                           timeout=600)
        got = [l for l in r.stdout.splitlines() if l.startswith("PLAIN ")]
        if r.returncode != 0 or not got:
            emit(f"{who}: the tree at {tree} could not be timed (exit {r.returncode}): {r.stderr.strip().splitlines()[-1:] or r.stdout.strip().splitlines()[-1:]}")
        else:
            alone[who] = json.loads(got[0][6:])
    if alone:
        emit("the device tail without the option, alone in a process of its own (no host tail between its rounds), one process after the other:")
        for what in BATCHES:
            emit(f"  {what}")
            for who, times in alone.items():
                emit(f"      {who:26s} {_fmt(times[what])}")
    emit("from the vocoder's return to every request's PCM on the host, wall clock with a device sync:")
    for what, frames in BATCHES.items():
        voc, tails = _tails(frames, device, loudness=True)
        times, results, stats = _time_tails(tails, reps)
        same = all(a.dtype == b.dtype == np.int16 and np.array_equal(a, b) for a, b in zip(results["host+loudness"], results["device+loudness"]))
        emit(f"  {what}: {sum(voc.lens)} samples  (host and device give the same bytes with the option: {same})")
        for name, _ in tails:
            st = stats[name]
            emit(f"      {name:26s} {_fmt(times[name])}   device-to-host copies: {st.get('d2h_copies', 0)}   wave_loudness calls: {st.get('loudness_calls', 0)}")
        extra = statistics.median(times["device+loudness"]) - statistics.median(times["device"])
        emit(f"      the option costs {extra * 1e3:.3f} ms of the device tail; the host tail with it is "
             f"{statistics.median(times['host+loudness']) / statistics.median(times['device+loudness']):.1f} x the device tail with it")
    emit("the library call alone, on PCM that is already on the device:")
    macs = 0.0
    for what, frames in BATCHES.items():
        m = library_call(what, frames, reps, device, emit)
        macs = macs or m
    if ARGS.kernel_db:
        kernel_db(ARGS.kernel_db, macs, emit)
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
