#!/usr/bin/env python3
"""What a per-request tempo and pitch cost: the host definition `wave_codec.shift_pcm16` against the device call `ops.wave_prosody`.

    python tools/wave_prosody_bench.py [--reps 9] [--out profiles/wave_prosody_bench.txt] [--parent TREE] [--variant LABEL=TREE]

Both sides run in ONE run and start from the requests' 24 kHz int16 PCM on the host and end with every request's shifted PCM on the host:
     host     `shift_pcm16` of each request, one after the other (numpy)
     device   the packed PCM goes up, ONE `ops.wave_prosody` call (two launches, one without a pitch), the packed result comes down
for one request of 10 s and for eight, with tempo 1.25 alone and with tempo 1.25 and pitch +2.  Wall clock with a device sync, median and
min .. max of `--reps` after a warm-up round.  Then the library call alone on PCM that is already on the device, in HIP events: the call
with tempo alone is the WSOLA launch (and the request table's copy), the call with the pitch both launches.  With the pitch the stretch is
184/205 instead of 4/5 and the WSOLA launch places 450 frames instead of 401, so the pitch launch is both launches minus the WSOLA launch
scaled by 450/401; the WSOLA launch also per frame of 480 output samples -- one workgroup, hence one CU, per request by construction, so
eight requests take the time of one.

`--parent TREE`: a checkout of the parent commit, built; the device tail WITHOUT the options -- `finish_requests(device_backend=True)` on
eight requests of one 10 s chunk each, chunk waves on the device -- is timed in child processes that run nothing else: the parent's tree,
this tree, the parent's again (the spread between the two parent runs is the noise).  `--variant LABEL=TREE`: another build of this tree
(a kernel variant under measurement); the device call's event times are taken in a child process from it as well.
`--tree TREE`: import the package from TREE (what a child process is given).

Nothing is decided by this file: no default follows from it and no threshold is set."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_args = argparse.ArgumentParser()
_args.add_argument("--reps", type=int, default=9)
_args.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_prosody_bench.txt"))
_args.add_argument("--parent", default=None)
_args.add_argument("--variant", action="append", default=[])
_args.add_argument("--tree", default=ROOT)
_args.add_argument("--child", choices=("tail", "call"), default=None, help="time one part alone and print one JSON line")
ARGS = _args.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import infer  # noqa: E402

RATE, SECONDS = 24000, 10
CASES = {"tempo 1.25": (1.25, 0), "tempo 1.25, pitch +2": (1.25, 2)}
COUNTS = (1, 8)


def _speech_like(n, seed, amp=0.12):
    g = np.random.default_rng(seed)
    t = np.arange(n) / float(RATE)
    w = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(g.uniform(80, 4000, 8), g.uniform(0, 2 * np.pi, 8))) / np.sqrt(8)
    env = 0.6 + 0.4 * np.sin(2 * np.pi * 2.7 * t + seed)
    return (amp * env * w + 0.01 * g.standard_normal(n)).astype(np.float32)


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


def call_times(reps):
    """{case: {count: event stats}} of `ops.wave_prosody` alone, the PCM already on the device."""
    from tts_indic_server_f5_amd import ops, wave_codec
    dev = torch.device("cuda:0")
    out = {}
    for name, (tempo, pitch) in CASES.items():
        spec = wave_codec.WaveSpec.of(dict(tempo=tempo, pitch=pitch))
        out[name] = {}
        for count in COUNTS:
            pcms = [infer.quantise_pcm16(_speech_like(SECONDS * RATE, s)) for s in range(count)]
            buf, offsets = _packed(pcms)
            pcm = torch.from_numpy(buf).to(dev)
            lens = [len(x) for x in pcms]
            out[name][str(count)] = _events(lambda: ops.wave_prosody(pcm, offsets, lens, None, [spec.stretch] * count, [pitch] * count), reps)
    return out


def tail_times(reps):
    """Event-free wall clock of the device tail without the options: eight requests of one 10 s chunk, chunk waves on the device."""
    dev = torch.device("cuda:0")
    chunks = [[torch.from_numpy(_speech_like(SECONDS * RATE, s)).to(dev)] for s in range(8)]
    return _wall(lambda: infer.finish_requests(chunks, ["x"] * 8, infer.cross_fade_duration, [False] * 8, device_backend=True, want="pcm16"), reps)


def _child(tree, part):
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--child", part, "--reps", str(ARGS.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if ARGS.child:
        print(json.dumps(tail_times(ARGS.reps) if ARGS.child == "tail" else call_times(ARGS.reps)))
        return
    from tts_indic_server_f5_amd import ops, wave_codec
    dev = torch.device("cuda:0")
    lines = [f"# tools/wave_prosody_bench.py on {torch.cuda.get_device_name(0)}: median ms (min .. max) of {ARGS.reps} after a warm-up round; requests of {SECONDS} s",
             "", "host shift_pcm16 against the device call, PCM on the host at both ends (upload and download included)",
             f"  {'case':24s} {'requests':8s} {'host':>32s} {'device':>32s}   host / device"]
    for name, (tempo, pitch) in CASES.items():
        spec = wave_codec.WaveSpec.of(dict(tempo=tempo, pitch=pitch))
        for count in COUNTS:
            pcms = [infer.quantise_pcm16(_speech_like(SECONDS * RATE, s)) for s in range(count)]
            buf, offsets = _packed(pcms)
            lens = [len(x) for x in pcms]
            host_out = []

            def host():
                host_out[:] = [wave_codec.shift_pcm16(x, tempo, pitch) for x in pcms]

            dev_out = []

            def device():
                pcm2, lengths2, offsets2, bounds2 = ops.wave_prosody(torch.from_numpy(buf).to(dev), offsets, lens, None, [spec.stretch] * count, [pitch] * count)
                down = pcm2.cpu().numpy()
                dev_out[:] = [down[o:o + b] for o, b in zip(offsets2, bounds2)]      # (no silence removal: a bound is the length)

            d = _wall(device, ARGS.reps)
            t0 = time.perf_counter()
            reps_host = max(3, ARGS.reps if count == 1 else 3)                        # the host side of eight requests takes seconds a round
            h = _wall(host, reps_host)
            assert all(np.array_equal(a, b) for a, b in zip(host_out, dev_out)), "the device call does not equal the host definition"
            lines.append(f"  {name:24s} {count:<8d} {_fmt(h):>32s} {_fmt(d):>32s}   {h['median'] / d['median']:.1f}" + (f"   (host: {reps_host} rounds)" if reps_host != ARGS.reps else ""))
            print(lines[-1], f"[{time.perf_counter() - t0:.1f} s]", flush=True)
    frames = -(-(-(-SECONDS * RATE * 4 // 5)) // 480) + 1
    frames_pitch = -(-(-(-SECONDS * RATE * 184 // 205)) // 480) + 1
    lines += ["", "the library call alone in HIP events, PCM on the device (the request table's copy and its wait included)",
              f"  {'build':12s} {'requests':8s} {'tempo alone = WSOLA launch':>32s} {'us per frame':>13s} {'with pitch +2 = both launches':>32s} "
              f"{f'pitch launch = both - WSOLA x {frames_pitch}/{frames}':>36s}"]
    builds = [("this tree", call_times(ARGS.reps))] + [(v.split("=", 1)[0], _child(v.split("=", 1)[1], "call")) for v in ARGS.variant]
    for label, t in builds:
        for count in COUNTS:
            a, b = t["tempo 1.25"][str(count)], t["tempo 1.25, pitch +2"][str(count)]
            lines.append(f"  {label:12s} {count:<8d} {_fmt(a):>32s} {1e3 * a['median'] / frames:13.2f} {_fmt(b):>32s} {b['median'] - a['median'] * frames_pitch / frames:36.3f}")
            print(lines[-1], flush=True)
    lines.append(f"  ({frames} frames of 480 output samples per request at tempo 1.25; with the pitch the stretch is 184/205 and the WSOLA launch places "
                 f"{frames_pitch} frames)")
    if ARGS.parent:
        lines += ["", "the device tail WITHOUT the options (finish_requests(device_backend=True), 8 requests of one 10 s chunk), each alone in a process"]
        for label, tree in (("parent 1", ARGS.parent), ("this tree", ROOT), ("parent 2", ARGS.parent)):
            lines.append(f"  {label:12s} {_fmt(_child(tree, 'tail'))}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    main()
