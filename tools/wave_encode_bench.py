#!/usr/bin/env python3
"""What the delivery format costs: from a micro-batch's vocoded chunks to every request's samples at another rate / in G.711 on the host.

    python tools/wave_encode_bench.py [--reps 9] [--out profiles/wave_encode_bench.txt]

The clock starts when the vocoder returns -- a stand-in `decode_ragged` hands out views of one packed fp32 buffer that is already on the
device, as F5HipVocos does -- and stops when every request's delivery-format samples are on the host.  Two tails, alternating in one process:
     host    `finish_requests(device_backend=False, sample_rate=..., encoding=...)`: the chunk waves come down, then join, quantisation,
             `resample_pcm16` and `encode_g711` in numpy
     device  `finish_requests(device_backend=True, ...)`: ONE f5hip_wave_finish call, ONE f5hip_wave_encode call behind it on the same
             stream, one download of the encoded samples
Cases: a micro-batch of 1 request and of 8 requests of one chunk of about 10 s, delivered as 8 kHz mu-law and as 44.1 kHz 16-bit PCM.  Wall
clock with a device sync, median and min..max of `--reps` (at least 7) after a warm-up round.  Bytes downloaded per request: what crosses
from the device on each path (`infer.backend_stats` counts the copies; the bytes follow from the shapes).

Nothing is decided by this file: `serve.DEVICE_BACKEND_DEFAULT` stays as it is, and no threshold is set."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import infer  # noqa: E402

HOP, FRAMES = 256, 938          # a chunk of (FRAMES - 1) * HOP = 239 872 samples, about 10 s


def _speech_like(n, seed, amp=0.12):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    w = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(g.uniform(80, 4000, 8), g.uniform(0, 2 * np.pi, 8))) / np.sqrt(8)
    return (amp * w + 0.01 * g.standard_normal(n)).astype(np.float32)


class PackedVocoder:
    """`decode_ragged` as F5HipVocos answers it: views of one packed device buffer, which is made before the clock starts"""

    def __init__(self, n_chunks, device):
        self.n = (FRAMES - 1) * HOP
        self.packed = torch.from_numpy(np.concatenate([_speech_like(self.n, 7 + i) for i in range(n_chunks)])).to(device)

    def decode_ragged(self, mels):
        return list(self.packed.split([self.n] * len(mels)))


def _fmt(ts):
    return f"{statistics.median(ts) * 1e3:8.3f} ms  ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})"


def case(n_req, rate, enc, reps, device, emit):
    voc = PackedVocoder(n_req, device)
    mel = torch.zeros(FRAMES, 100, device=device)
    groups = [([mel], 0, torch.tensor(0.2))] * n_req
    texts = ["x"] * n_req

    def host():
        waves = [w for w, _ in infer._chunk_waves(groups, voc, "vocos", infer.target_rms, want_specs=False)]
        return infer.finish_requests(waves, texts, infer.cross_fade_duration, want="pcm16", sample_rate=rate, encoding=enc)

    def dev():
        waves = [w for w, _ in infer._chunk_waves(groups, voc, "vocos", infer.target_rms, on_device=True, want_specs=False)]
        return infer.finish_requests(waves, texts, infer.cross_fade_duration, device_backend=True, want="pcm16", sample_rate=rate, encoding=enc)

    tails = (("host", host), ("device", dev))
    times, copies, results = {name: [] for name, _ in tails}, {}, {}
    for rep in range(reps + 1):                      # the first round warms both up (workspaces, tap tables, allocator, numpy buffers)
        for name, fn in tails:
            infer.backend_stats.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
            copies[name] = infer.backend_stats["d2h_copies"]
    same = all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(results["host"], results["device"]))
    down = {"host": 4 * voc.n, "device": results["device"][0].nbytes}      # fp32 chunk wave | the encoded samples
    emit(f"  {n_req} x 10 s -> {rate} Hz {enc}  (both tails give the same bytes: {same})")
    for name, _ in tails:
        emit(f"      {name:7s} {_fmt(times[name])}   device-to-host copies per batch: {copies[name]}   bytes downloaded per request: {down[name]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wave_encode_bench.txt"))
    args = ap.parse_args()
    reps = max(args.reps, 7)
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    assert torch.cuda.is_available(), "needs a HIP device"
    device = torch.device("cuda:0")
    emit(f"tools/wave_encode_bench.py: median (min .. max) of {reps}, wall clock with a device sync, from the vocoder's return to the delivery-format samples on the host")
    emit(f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")
    for n_req in (1, 8):
        for rate, enc in ((8000, "mulaw"), (44100, "pcm16")):
            case(n_req, rate, enc, reps, device, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
