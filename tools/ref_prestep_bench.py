#!/usr/bin/env python3
"""What the silence pre-step of an uploaded reference clip costs: the host function against the device call, in the same run.

    python tools/ref_prestep_bench.py [--reps 9] [--out profiles/ref_prestep_bench.txt]

1. The pre-step alone, from the clip's int16 frames on the host: one 30 s 44.1 kHz mono clip (the clip of
   profiles/ref_frontend_prestep_cpu.txt), then eight such clips in stereo.
     host    `audio_prep.preprocess_ref_segment`, clip by clip (a fresh PcmSegment each time: nothing cached)
     device  `ops.ref_prestep`: one upload of the packed frames, ONE f5hip_ref_prestep call (three launches), one download of the lengths
             and flags; the samples stay on the device
2. `TTSManager._clip_voice` end to end on a fresh 30 s 44.1 kHz stereo upload (hash, quantise, pre-step, the deferred voice), with and
   without `device_prestep`, both with `device_frontend`.
Wall clock with a device sync, the two sides alternating in one process, median and min..max of `--reps` (at least 9) after a warm-up.
The first repetition also checks that the device result equals the host one."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import audio_prep, ops, serve, synth  # noqa: E402

SR, SECONDS = 44100, 30.0
PAUSES = ((0.0, 0.4), (4.0, 4.3), (9.5, 10.8), (14.0, 14.2), (21.0, 22.5), (29.5, 30.0))      # seconds, as tools/ref_frontend_bench.py


def _speech_like(n, sr, seed, amp=0.2):
    g = np.random.default_rng(seed)
    t = np.arange(n) / sr
    w = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip(g.uniform(80, 4000, 8), g.uniform(0, 2 * np.pi, 8))) / np.sqrt(8)
    return (amp * w + 0.01 * g.standard_normal(n)).astype(np.float32)


def _clip(channels, seed):
    """int16 frames [n, channels] of the 30 s clip"""
    n = int(SR * SECONDS)
    gate = np.ones(n, dtype=np.float32)
    for a, b in PAUSES:
        gate[int(a * SR):int(b * SR)] = 0.0
    x = np.stack([_speech_like(n, SR, seed + 31 * c) * gate for c in range(channels)], axis=1)
    return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)


def _fmt(ts):
    return f"{statistics.median(ts) * 1e3:8.3f} ms  ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})"


def pre_step(reps, emit, device):
    for label, n, ch in (("one clip, 30 s 44.1 kHz mono", 1, 1), ("eight clips, 30 s 44.1 kHz stereo", 8, 2)):
        clips = [_clip(ch, seed=7 + 100 * i) for i in range(n)]
        frames = np.concatenate([c.reshape(-1) for c in clips])
        times = {"host": [], "device": []}
        for rep in range(reps + 1):                              # the first round warms both up (workspaces, allocator)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = [audio_prep.preprocess_ref_segment(audio_prep.PcmSegment(c, SR), True, show_info=lambda *_: None) for c in clips]
            t1 = time.perf_counter()
            packed, lengths, flags = ops.ref_prestep(frames, [c.shape[0] for c in clips], [ch] * n, SR, True, device=device)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep:
                times["host"].append(t1 - t0)
                times["device"].append(t2 - t1)
            else:
                want = np.concatenate([(s.frames.astype(np.float32) / 32768.0).T.reshape(-1) for s in host])
                assert lengths == [s.frames.shape[0] for s in host] and all(flags) and np.array_equal(packed.cpu().numpy(), want)
        emit(f"  {label}:")
        emit(f"    host    preprocess_ref_segment, clip by clip     {_fmt(times['host'])}")
        emit(f"    device  ops.ref_prestep, upload and download in  {_fmt(times['device'])}")
        yield statistics.median(times["host"]), statistics.median(times["device"])


def clip_voice(model, reps, emit):
    mgrs = {flag: serve.TTSManager(device_frontend=True, device_prestep=flag, clip_cache=2) for flag in (True, False)}
    for mgr in mgrs.values():
        mgr.model_obj = model
    times = {True: [], False: []}
    for rep in range(reps + 1):
        wave = torch.from_numpy(np.ascontiguousarray(_clip(2, seed=1000 + rep).T.astype(np.float32) / 32768.0))      # a new upload every repetition
        for flag, mgr in mgrs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            voice, _ = mgr._clip_voice((wave, SR), "some words")
            torch.cuda.synchronize()
            if rep:
                times[flag].append(time.perf_counter() - t0)
            assert voice.pending is not None and voice.pending[0].is_cuda == flag
    emit("  _clip_voice, one fresh 30 s 44.1 kHz stereo upload (hash, quantise, pre-step, deferred voice):")
    emit(f"    device_prestep=True   {_fmt(times[True])}")
    emit(f"    device_prestep=False  {_fmt(times[False])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ref_prestep_bench.txt"))
    args = ap.parse_args()
    reps = max(args.reps, 9)
    lines = []

    def emit(line=""):
        print(line, flush=True)
        lines.append(line)

    assert torch.cuda.is_available(), "needs a HIP device"
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    arch = dict(dim=256, depth=2, heads=4, ff_mult=2, text_dim=64, conv_layers=2, text_num_embeds=40)
    model = F5HipModel(DiTArch(**arch), synth.dit_state_dict(**arch))            # (only its device is used: no request is sampled here)
    emit(f"tools/ref_prestep_bench.py: median (min .. max) of {reps}, wall clock with a device sync")
    emit(f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")
    emit("1. the pre-step alone, from int16 frames on the host (device: upload + f5hip_ref_prestep + download of lengths and flags)")
    results = list(pre_step(reps, emit, model.device))
    host8, dev8 = results[-1]
    emit(f"   eight clips: the device call {'beats' if dev8 < host8 else 'does NOT beat'} the host function ({host8 / dev8:.2f} x); "
         "the option stays off by default either way")
    emit("2. the serving path")
    clip_voice(model, reps, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
