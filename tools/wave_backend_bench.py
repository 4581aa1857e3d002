#!/usr/bin/env python3
"""What it costs to turn a micro-batch's vocoded chunks into finished 16-bit PCM: the host tail against the device back-end.

    python tools/wave_backend_bench.py [--reps 9] [--out profiles/wave_backend_bench.txt]

The clock starts when the vocoder returns -- a stand-in `decode_ragged` hands out views of one packed fp32 buffer that is already on the
device, as F5HipVocos does -- and stops when every request's int16 PCM is on the host.  Three tails, alternating in one process:
     before  the serving path as it was: `_chunk_waves` downloads every chunk wave and every chunk spectrogram, then per request
             `request_wave` (float64 cross-fade, float32 cast) and the routes' quantisation (`wav_bytes`)
     host    `finish_requests(device_backend=False)`: the same arithmetic, the spectrograms no longer downloaded
     device  `finish_requests(device_backend=True)`: the waves stay on the device, ONE f5hip_wave_finish call, one download of the samples
             (and one of the lengths when a request asked for silence removal)
Cases: 1 request x 1 chunk, 8 x 2 and 16 x 3 chunks of about 10 s, each without and with `remove_silence` (every chunk holds a 1.2 s
pause).  Wall clock with a device sync, median and min..max of `--reps` (at least 7) after a warm-up round; device-to-host copies per batch
are counted by `infer.backend_stats`.  The reference voice's rms is above the target, so no gain is applied (the usual prepared voice).

Whether the back-end may become the default (`serve.DEVICE_BACKEND_DEFAULT`) follows from the 1 x 1 cases: only if the device tail beats
the host one by more than the spread (max - min) of either in the same run."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import audio_prep, infer  # noqa: E402

HOP, FRAMES = 256, 938          # a chunk of (FRAMES - 1) * HOP = 239 872 samples, about 10 s


def _speech_like(n, seed, amp=0.12):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    w = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(g.uniform(80, 4000, 8), g.uniform(0, 2 * np.pi, 8))) / np.sqrt(8)
    x = (amp * w + 0.01 * g.standard_normal(n)).astype(np.float32)
    a = int(g.integers(n // 4, n // 2))
    x[a:a + 28800] = 0.0         # a 1.2 s pause
    return x


class PackedVocoder:
    """`decode_ragged` as F5HipVocos answers it: views of one packed device buffer, which is made before the clock starts"""

    def __init__(self, n_chunks, device):
        self.n = (FRAMES - 1) * HOP
        self.packed = torch.from_numpy(np.concatenate([_speech_like(self.n, 7 + i) for i in range(n_chunks)])).to(device)

    def decode_ragged(self, mels):
        return list(self.packed.split([self.n] * len(mels)))


def _fmt(ts):
    return f"{statistics.median(ts) * 1e3:8.3f} ms  ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})"


def case(n_req, n_chunks, cut, reps, device, emit):
    voc = PackedVocoder(n_req * n_chunks, device)
    mel = torch.zeros(FRAMES, 100, device=device)
    groups = [([mel] * n_chunks, 0, torch.tensor(0.2))] * n_req
    texts, flags = ["x"] * n_req, [cut] * n_req

    def before():
        out = []
        for waves, _ in infer._chunk_waves(groups, voc, "vocos", infer.target_rms):
            pcm = infer.quantise_pcm16(infer.request_wave("x", waves))
            out.append(audio_prep.remove_silence_pcm(pcm) if cut else pcm)
        return out

    def host():
        waves = [w for w, _ in infer._chunk_waves(groups, voc, "vocos", infer.target_rms, want_specs=False)]
        return infer.finish_requests(waves, texts, infer.cross_fade_duration, flags, want="pcm16")

    def dev():
        waves = [w for w, _ in infer._chunk_waves(groups, voc, "vocos", infer.target_rms, on_device=True, want_specs=False)]
        return infer.finish_requests(waves, texts, infer.cross_fade_duration, flags, device_backend=True, want="pcm16")

    tails = (("before", before), ("host", host), ("device", dev))
    times, copies, results = {name: [] for name, _ in tails}, {}, {}
    for rep in range(reps + 1):                      # the first round warms all three up (workspaces, allocator, numpy buffers)
        for name, fn in tails:
            infer.backend_stats.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
            copies[name] = infer.backend_stats["d2h_copies"]
    same = all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(results["before"], results["host"], results["device"]))
    emit(f"  {n_req:2d} x {n_chunks} chunks of 10 s, remove_silence {'on ' if cut else 'off'}  (the three tails give the same samples: {same})")
    for name, _ in tails:
        emit(f"      {name:7s} {_fmt(times[name])}   device-to-host copies per batch: {copies[name]}")
    h, d = times["host"], times["device"]
    return statistics.median(h) - statistics.median(d) > max(max(h) - min(h), max(d) - min(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wave_backend_bench.txt"))
    args = ap.parse_args()
    reps = max(args.reps, 7)
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    assert torch.cuda.is_available(), "needs a HIP device"
    device = torch.device("cuda:0")
    emit(f"tools/wave_backend_bench.py: median (min .. max) of {reps}, wall clock with a device sync, from the vocoder's return to int16 PCM on the host")
    emit(f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")
    verdicts = []
    for n_req, n_chunks in ((1, 1), (8, 2), (16, 3)):
        for cut in (False, True):
            won = case(n_req, n_chunks, cut, reps, device, emit)
            if n_req == 1:
                verdicts.append(won)
    emit(f"1 x 1: the device tail beats the host tail by more than the run's spread in {sum(verdicts)} of {len(verdicts)} cases")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
