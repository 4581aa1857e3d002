#!/usr/bin/env python3
"""What a per-request `keep_formants` costs: the host definition `wave_codec.shift_pcm16(..., keep_formants=True)` against the device call
`ops.wave_prosody(..., keep_formants=...)`.

    python tools/wave_formant_bench.py [--reps 9] [--out profiles/wave_formant_bench.txt] [--parent TREE] [--kernel-db DB]

Both sides run in ONE run and start from the requests' 24 kHz int16 PCM on the host and end with every request's shifted PCM on the host:
     host     `shift_pcm16` of each request, one after the other (numpy)
     device   the packed PCM goes up, ONE `ops.wave_prosody` call (WSOLA and the three launches of csrc/wave_formant.h), the packed result
              comes down
for one request of 10 s and for eight, at pitch +4 kept, without a tempo and with tempo 1.25.  Wall clock with a device sync, median and
min .. max of `--reps` after a warm-up round.  Then the library call alone on PCM that is already on the device, in HIP events: the flagged
call, and the same call without the flags and without a pitch (the WSOLA launch alone: a copy at tempo 1.0), so their difference is the three
new launches together.  The call is one C entry, so events cannot go between its launches: the three launches one by one come from a
`rocprofv3 --kernel-trace` run of `--trace-loop N` (N calls on one request, then N on eight, pitch +4 kept, and nothing else), whose rocpd
database `--kernel-db DB` reads.

`--parent TREE`: a checkout of the parent commit, built; the device tail WITHOUT the option -- `finish_requests(device_backend=True)` on
eight requests of one 10 s chunk each, chunk waves on the device -- is timed in child processes that run nothing else: the parent's tree,
this tree, the parent's again (the spread between the two parent runs is the noise).  `--tree TREE`: import the package from TREE (what a
child process is given).

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
_args.add_argument("--reps", type=int, default=9)
_args.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_formant_bench.txt"))
_args.add_argument("--parent", default=None)
_args.add_argument("--kernel-db", default=None)
_args.add_argument("--trace-loop", type=int, default=0)
_args.add_argument("--tree", default=ROOT)
_args.add_argument("--child", choices=("tail",), default=None, help="time one part alone and print one JSON line")
ARGS = _args.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import infer  # noqa: E402

RATE, SECONDS, PITCH = 24000, 10, 4
CASES = {"pitch +4 kept": 1.0, "tempo 1.25, pitch +4 kept": 1.25}
COUNTS = (1, 8)
KERNELS = ("wave_wsola_kernel", "wave_period_kernel", "wave_marks_kernel", "wave_psola_kernel")


def _speech_like(n, seed, amp=0.12):
    """Voiced stretches (harmonics of a gliding 100 .. 220 Hz fundamental under a slow envelope), noise between them."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / float(RATE)
    f0 = g.uniform(100, 220) * (1.0 + 0.15 * np.sin(2 * np.pi * 0.4 * t + seed))
    phase = 2 * np.pi * np.cumsum(f0) / RATE
    voiced = sum(np.sin(h * phase + p) / h for h, p in zip(range(1, 13), g.uniform(0, 2 * np.pi, 12)))
    gate = (np.sin(2 * np.pi * 0.7 * t + seed) > -0.3).astype(np.float64)
    return (amp * (gate * voiced / 2.0 + (1.0 - gate) * 0.3 * g.standard_normal(n)) + 0.002 * g.standard_normal(n)).astype(np.float32)


def _stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def _fmt(s):
    return f"{s['median']:9.3f} ({s['min']:.3f} .. {s['max']:.3f})"


def _wall(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return _stats(out)


def _events(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return _stats(out)


def _packed(pcms):
    offsets, off = [], 0
    for x in pcms:
        offsets.append(off)
        off += (len(x) + 7) & ~7
    buf = np.zeros(off, dtype=np.int16)
    for o, x in zip(offsets, pcms):
        buf[o:o + len(x)] = x
    return buf, offsets


def _requests(count):
    pcms = [infer.quantise_pcm16(_speech_like(SECONDS * RATE, s)) for s in range(count)]
    buf, offsets = _packed(pcms)
    return pcms, buf, offsets, [len(x) for x in pcms]


def tail_times(reps):
    """Event-free wall clock of the device tail without the option: eight requests of one 10 s chunk, chunk waves on the device."""
    dev = torch.device("cuda:0")
    chunks = [[torch.from_numpy(_speech_like(SECONDS * RATE, s)).to(dev)] for s in range(8)]
    return _wall(lambda: infer.finish_requests(chunks, ["x"] * 8, infer.cross_fade_duration, [False] * 8, device_backend=True, want="pcm16"), reps)


def _child(tree, part):
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--child", part, "--reps", str(ARGS.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_db(path, emit):
    """Per kernel and grid of the trace: launches, median and range.  One request and eight differ by their grids."""
    rows = sqlite3.connect(path).execute("select name, grid_x, workgroup_x, duration from kernels").fetchall()
    emit(f"kernel times of a rocprofv3 --kernel-trace run of --trace-loop ({os.path.basename(path)}): pitch +4 kept, no tempo")
    emit(f"  {'kernel':20s} {'workgroups':>10s} {'launches':>8s} {'median us':>10s}   (min .. max)")
    for key in KERNELS:
        grids = sorted({gx // max(wx, 1) for name, gx, wx, _ in rows if key in name})
        if not grids:
            emit(f"  {key}: not in the trace")
        for grid in grids:
            d = sorted(d for name, gx, wx, d in rows if key in name and gx // max(wx, 1) == grid)
            emit(f"  {key:20s} {grid:10d} {len(d):8d} {d[len(d) // 2] * 1e-3:10.1f}   ({d[0] * 1e-3:.1f} .. {d[-1] * 1e-3:.1f})")


def main():
    if ARGS.child:
        print(json.dumps(tail_times(ARGS.reps)))
        return
    from tts_indic_server_f5_amd import ops, wave_codec
    dev = torch.device("cuda:0")
    if ARGS.trace_loop:
        for count in COUNTS:
            _, buf, offsets, lens = _requests(count)
            pcm = torch.from_numpy(buf).to(dev)
            for _ in range(ARGS.trace_loop):
                ops.wave_prosody(pcm, offsets, lens, None, [(1, 1)] * count, [PITCH] * count, keep_formants=[True] * count)
            torch.cuda.synchronize()
        return
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    emit(f"# tools/wave_formant_bench.py on {torch.cuda.get_device_name(0)}: median ms (min .. max) of {ARGS.reps} after a warm-up round; requests of {SECONDS} s")
    emit()
    emit("host shift_pcm16(..., keep_formants=True) against the device call, PCM on the host at both ends (upload and download included)")
    emit(f"  {'case':28s} {'requests':8s} {'host':>34s} {'device':>32s}   host / device")
    for name, tempo in CASES.items():
        stretch = wave_codec.formant_stretch(round(100 * tempo))
        for count in COUNTS:
            pcms, buf, offsets, lens = _requests(count)
            host_out, dev_out = [], []

            def host():
                host_out[:] = [wave_codec.shift_pcm16(x, tempo, PITCH, keep_formants=True) for x in pcms]

            def device():
                pcm2, _, offsets2, bounds2 = ops.wave_prosody(torch.from_numpy(buf).to(dev), offsets, lens, None, [stretch] * count, [PITCH] * count,
                                                              keep_formants=[True] * count)
                down = pcm2.cpu().numpy()
                dev_out[:] = [down[o:o + b] for o, b in zip(offsets2, bounds2)]      # (no silence removal: a bound is the length)

            d = _wall(device, ARGS.reps)
            reps_host = max(3, ARGS.reps if count == 1 else 3)                        # the host side of eight requests takes seconds a round
            h = _wall(host, reps_host)
            assert all(np.array_equal(a, b) for a, b in zip(host_out, dev_out)), "the device call does not equal the host definition"
            moved = sum(int((a != x[:len(a)]).sum()) if len(a) == len(x) else -1 for a, x in zip(host_out, pcms))
            emit(f"  {name:28s} {count:<8d} {_fmt(h):>34s} {_fmt(d):>32s}   {h['median'] / d['median']:.1f}" + (f"   (host: {reps_host} rounds)" if reps_host != ARGS.reps else "")
                 + (f"   [{moved} samples changed]" if moved >= 0 else ""))
    emit()
    emit("the library call alone in HIP events, PCM on the device (the request tables' copies and their waits included)")
    emit(f"  {'case':28s} {'requests':8s} {'flagged call':>32s} {'WSOLA launch alone':>32s}   the three launches (difference of the medians)")
    for name, tempo in CASES.items():
        stretch = wave_codec.formant_stretch(round(100 * tempo))
        for count in COUNTS:
            _, buf, offsets, lens = _requests(count)
            pcm = torch.from_numpy(buf).to(dev)
            a = _events(lambda: ops.wave_prosody(pcm, offsets, lens, None, [stretch] * count, [PITCH] * count, keep_formants=[True] * count), ARGS.reps)
            b = _events(lambda: ops.wave_prosody(pcm, offsets, lens, None, [stretch] * count, [0] * count), ARGS.reps)
            emit(f"  {name:28s} {count:<8d} {_fmt(a):>32s} {_fmt(b):>32s}   {a['median'] - b['median']:.3f}")
    if ARGS.kernel_db:
        emit()
        kernel_db(ARGS.kernel_db, emit)
    if ARGS.parent:
        emit()
        emit("the device tail WITHOUT the option (finish_requests(device_backend=True), 8 requests of one 10 s chunk), each alone in a process")
        for label, tree in (("parent 1", ARGS.parent), ("this tree", ROOT), ("parent 2", ARGS.parent)):
            emit(f"  {label:12s} {_fmt(_child(tree, 'tail'))}")
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    main()
