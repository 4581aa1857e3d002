#!/usr/bin/env python3
"""Time to first audio and total time of `TTSManager.synthesize` vs `TTSManager.synthesize_stream`, plus the Vocos time of one
micro-batch of ragged chunks (per-chunk `decode` loop vs one `decode_ragged` call).

    python tools/stream_latency.py [--nfe 32] [--clients 1 8] [--reps 3]

Workload: F5-TTS Base width (synthetic weights), 32 NFE, CFG 2, sway -1, Vocos; a 5 s prompt and a text that chunks into three
units of about 1 400 frames each; a manager with the micro-batcher (max 16 requests, 5 ms window) and shape-invariant attention, as
served.  C clients start together (one thread each).  "first" = when the client holds its first samples: the whole wave unstreamed,
the first piece streamed; "total" = when it holds the last one.  Wall clock on the host, after one warm-up request per mode."""
import argparse
import os
import statistics
import sys
import tempfile
import threading
import time
import wave

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tts_indic_server_f5_amd import infer, serve, synth  # noqa: E402
from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel  # noqa: E402
from tts_indic_server_f5_amd.vocoder import F5HipVocos  # noqa: E402

VOCAB = {chr(32 + i): i for i in range(96)}   # printable ASCII
REF_TEXT = "Some call me nature, others call me mother nature."
# three sentences of ~105 bytes, no commas (chunk_text also splits there): two do not fit one chunk's byte budget, so each is a
# unit of ~1 400 frames
TEXT = ("I have been a silent spectator for billions of years and watched every species evolve and wander the land. "
        "I have seen great empires rise and fall and rivers change their course as the mountains wear down to dust. "
        "Always remember that I am mighty and enduring so respect me and I will nurture you for all of your days.")


def _prompt_wav(path, seconds=5.0):
    x = (synth.ref_audio(int(24000 * seconds)).numpy()[0] * 32767).astype(np.int16)
    with wave.open(path, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
        f.writeframes(x.tobytes())


def _client(mgr, path, streamed, start, out, i):
    start.wait()
    t0 = time.perf_counter()
    first = None
    n = 0
    if streamed:
        for piece in mgr.synthesize_stream(TEXT, ref_audio_path=path, ref_text=REF_TEXT):
            if first is None:
                first = time.perf_counter() - t0
            n += len(piece)
    else:
        n = len(mgr.synthesize(TEXT, ref_audio_path=path, ref_text=REF_TEXT))
        first = time.perf_counter() - t0
    out[i] = (first, time.perf_counter() - t0, n)


def run_clients(mgr, path, clients, streamed):
    start, out = threading.Event(), [None] * clients
    th = [threading.Thread(target=_client, args=(mgr, path, streamed, start, out, i)) for i in range(clients)]
    for t in th:
        t.start()
    start.set()
    for t in th:
        t.join()
    return out


def vocos_batch(voc, n_chunks, reps):
    g = torch.Generator().manual_seed(1)
    frames = [int(x) for x in torch.randint(700, 1400, (n_chunks,), generator=g)]
    mels = [(torch.randn(100, t, generator=g) * 1.5 - 1.0).cuda() for t in frames]
    res = {}
    for name, fn in (("per-chunk decode loop", lambda: [voc.decode(m[None]) for m in mels]), ("one decode_ragged call", lambda: voc.decode_ragged(mels))):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[name] = statistics.median(ts)
    return frames, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nfe", type=int, default=32)
    ap.add_argument("--clients", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=3, help="repetitions per (clients, mode); medians over all clients of all repetitions")
    ap.add_argument("--vocos-chunks", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    model = F5HipModel(F5TTS_BASE, synth.dit_state_dict(), vocab_char_map=VOCAB)
    voc = F5HipVocos(synth.vocos_state_dict())
    mgr = serve.TTSManager(nfe_step=args.nfe, micro_batch=dict(max_requests=16, max_wait_ms=5)).load(model, voc)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "prompt.wav")
        _prompt_wav(path)
        voice, ref_text_n = mgr._voice(path, REF_TEXT)
        chunks = infer.request_chunks(ref_text_n, voice.seconds, TEXT)
        units = infer.plan_units(ref_text_n + " ", chunks, voice.ref_frames)
        print(f"workload: F5-TTS Base, {args.nfe} NFE, CFG 2, sway -1, Vocos; prompt {voice.seconds:.2f} s; "
              f"{len(chunks)} chunks, unit frames {[f for _, f in units]}; micro-batcher max 16 requests / 5 ms; device {torch.cuda.get_device_name(0)}")
        for streamed in (False, True):                       # warm-up: workspaces at the largest batch, reference mel
            run_clients(mgr, path, max(args.clients), streamed)
        print(f"{'clients':>7} {'mode':>10} {'first audio median / max (s)':>30} {'total median / max (s)':>24}  samples")
        for c in args.clients:
            for streamed in (False, True):
                rows = [r for _ in range(args.reps) for r in run_clients(mgr, path, c, streamed)]
                firsts, totals = [r[0] for r in rows], [r[1] for r in rows]
                print(f"{c:>7} {'streamed' if streamed else 'whole':>10} {statistics.median(firsts):>16.3f} / {max(firsts):.3f}"
                      f" {statistics.median(totals):>14.3f} / {max(totals):.3f}  {rows[0][2]}", flush=True)
    mgr.close()
    frames, res = vocos_batch(voc, args.vocos_chunks, max(args.reps, 5))
    print(f"Vocos, one micro-batch of {len(frames)} chunks ({min(frames)}-{max(frames)} frames, {sum(frames)} total), median of "
          f"{max(args.reps, 5)}, wall clock with a device sync:")
    for name, t in res.items():
        print(f"  {name:24s} {t * 1e3:8.2f} ms")


if __name__ == "__main__":
    main()
