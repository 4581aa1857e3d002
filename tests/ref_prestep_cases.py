"""The case matrix of the reference-clip pre-step (audio_prep.preprocess_ref_segment / preprocess_ref_ranges / ops.ref_prestep), shared by
tests/test_ref_prestep_host.py, tests/test_ref_prestep_core.py and tests/test_gpu_ref_prestep.py.  Everything is deterministic: tones,
low-level noise from a seeded generator and constant-amplitude square waves (the rms of a +-a square wave is exactly a).  The long cases
are 11 025 Hz mono to stay small.  `cases()` -> {name: (int16 frames [n, channels], rate, clip_short)}."""
import functools
import math

import numpy as np

from tts_indic_server_f5_amd import audio_prep as AP


TRAIL_ROUNDING = {"trail_2500": (22050, 3000, 2500), "trail_9000": (11025, 600, 9000)}     # name: (rate, loud body ms, trailing silence ms)


def n_frames(ms, rate):
    return int(round(ms * rate / 1000.0))


def tone(ms, rate, amp=8000, hz=220.0, ch=1):
    t = np.arange(n_frames(ms, rate), dtype=np.float64) / rate
    x = np.rint(amp * np.sin(2 * np.pi * hz * t + 0.3))
    return np.stack([np.rint(x * (1.0 - 0.25 * c)) for c in range(ch)], axis=1).astype(np.int16)


def square(ms, rate, amp, ch=1):
    x = np.where(np.arange(n_frames(ms, rate)) % 2 == 0, amp, -amp)
    return np.repeat(x[:, None], ch, axis=1).astype(np.int16)


def noise(ms, rate, dbfs=-60.0, ch=1, seed=1):
    rng = np.random.default_rng(seed)
    a = 32768.0 * 10 ** (dbfs / 20.0) * math.sqrt(3.0)             # uniform in [-a, a] has rms a / sqrt(3)
    return np.rint(rng.uniform(-a, a, size=(n_frames(ms, rate), ch))).astype(np.int16)


def zeros(ms, rate, ch=1):
    return np.zeros((n_frames(ms, rate), ch), dtype=np.int16)


def cat(*parts):
    return np.concatenate(parts, axis=0)


def thresholds():
    """T of each rule, from the host rule itself: (pass 1, pass 2, edges): amplitude T counts as silent, T + 1 does not."""
    t1, t2 = (math.isqrt(AP.silence_square(db)) - 1 for _, db in AP.REF_CLIP_PASSES)
    lead, trail = AP.edge_rms_thresholds()
    assert lead == trail
    return t1, t2, lead - 1


@functools.lru_cache(maxsize=None)
def cases():
    R, out = 11025, {}
    # 1. short clips: uneven frames per millisecond, channel sums, edges only
    out["short_44100_stereo"] = (tone(3000, 44100, ch=2), 44100, True)
    out["short_22050_stereo"] = (tone(3000, 22050, ch=2), 22050, True)
    out["short_48000_mono"] = (tone(3000, 48000), 48000, True)
    # 2. degenerate clips
    out["zero_frames"] = (np.zeros((0, 1), dtype=np.int16), R, True)
    out["one_frame"] = (np.full((1, 1), 9000, dtype=np.int16), R, True)
    out["ms_99"] = (tone(99, R), R, True)
    out["ms_999"] = (tone(999, R, ch=2), R, True)
    out["zeros_2s"] = (zeros(2000, R), R, True)
    last = zeros(2000, R)
    last[-1, 0] = 12000
    out["last_sample_2s"] = (last, R, True)
    # 3. pass 1 stops at a pause: 20 s with pauses of 1.2 s at -60 dBFS; a variant whose first chunk alone is over 15 s
    pause = lambda ms, seed: noise(ms, R, -60.0, seed=seed)
    stop = cat(tone(3600, R), pause(1200, 2), tone(3500, R, hz=180.0), pause(1200, 3), tone(4200, R), pause(1200, 4), tone(3900, R, hz=300.0), pause(1200, 5))
    first_long = cat(tone(16000, R), pause(1200, 6), tone(2800, R))
    # 4. pass 2 is taken: pauses of 150 - 300 ms only, so pass 1 keeps one chunk of 20 s; pass 2's padded ranges overlap
    parts = []
    for i in range(11):
        parts += [tone(1550 + 37 * i, R, hz=200.0 + 10 * i), pause(150 + 15 * i, 10 + i)]
    short_pauses = cat(*parts)[:n_frames(20000, R)]
    # 5. hard cut: no pause at all
    no_pause = tone(20000, R)
    for name, x in (("pass1_stop", stop), ("pass1_first_chunk_long", first_long), ("pass2_short_pauses", short_pauses), ("hard_cut", no_pause)):
        out[name] = (x, R, True)
        out[name + "_noclip"] = (x, R, False)                                   # 9. clip_short=False on cases 3 - 5
    # 6. threshold pairs: a window amplitude at T and at T + 1
    t1, t2, te = thresholds()
    for a in (t1, t1 + 1):
        out[f"thresh_pass1_{a}"] = (cat(tone(1500, R), square(2600, R, a), tone(1500, R)), R, True)
    for a in (t2, t2 + 1):
        out[f"thresh_pass2_{a}"] = (cat(tone(9000, R), square(2600, R, a), tone(8400, R)), R, True)
    for a in (te, te + 1):
        out[f"thresh_edges_{a}"] = (cat(square(500, R, a, ch=2), tone(1000, R, ch=2), square(300, R, a, ch=2)), R, True)
    # 7. the extra window: (len_ms - min_silence_len) % 10 != 0, once per parameter set, each ending in a pause the extra window sees
    out["extra_window_pass1"] = (cat(tone(3600, R), pause(1200, 2), tone(4000, R), pause(1007, 7)), R, True)
    out["extra_window_pass2"] = (cat(short_pauses[:n_frames(19800, R)], pause(203, 8)), R, True)
    # 8. edges: leading silences of 37 and 1 234 ms, trailing ones of 2.5 and 9 s, both on a clipped concatenation of two ranges
    out["lead_37"] = (cat(zeros(37, R), tone(1500, R)), R, True)
    out["lead_1234"] = (cat(zeros(1234, R), tone(1500, R)), R, True)
    # (TRAIL_ROUNDING: a loud body of a whole number of frames, then zeros; exact arithmetic would keep body_ms, the running subtraction
    # of 0.001 ends just below it and keeps body_ms - 1)
    for name, (rate, body_ms, quiet_ms) in TRAIL_ROUNDING.items():
        out[name] = (cat(square(body_ms, rate, 8000), zeros(quiet_ms, rate)), rate, False)
    out["edges_two_ranges"] = (cat(pause(1234, 11), tone(3000, R), pause(3000, 12), tone(2500, R), pause(2500, 13)), R, True)
    out["edges_two_ranges_44100"] = (cat(zeros(37, 44100, 2), tone(1200, 44100, ch=2), zeros(2600, 44100, 2), tone(900, 44100, ch=2), noise(1100, 44100, -55.0, 2, 14)),
                                     44100, True)
    return out


def segment(name):
    x, rate, clip = cases()[name]
    return AP.PcmSegment(x, rate), clip


@functools.lru_cache(maxsize=None)
def expected(name):
    """The frames of preprocess_ref_segment for a case: the reference every test compares against, computed once."""
    seg, clip = segment(name)
    out = AP.preprocess_ref_segment(seg, clip, show_info=lambda *_: None).frames
    out.setflags(write=False)
    return out


def random_layout(seed):
    """A seeded random pause / level / rate / channel layout: (frames, rate, clip_short)."""
    rng = np.random.default_rng(1000 + seed)
    rate = int(rng.choice([11025, 12000, 16000, 22050]))
    ch = int(rng.choice([1, 1, 2, 3]))
    t1, t2, te = thresholds()
    parts, total, want = [], 0, int(rng.choice([700, 2500, 9000, 17000, 21000]))
    while total < want:
        kind = int(rng.integers(0, 6))
        ms = int(rng.choice([3, 40, 130, 260, 700, 1100, 1600, 2300, 4100]))
        if kind <= 1:
            parts.append(tone(ms, rate, amp=int(rng.integers(400, 12000)), hz=float(rng.integers(100, 900)), ch=ch))
        elif kind == 2:
            parts.append(zeros(ms, rate, ch))
        elif kind == 3:
            parts.append(noise(ms, rate, float(rng.uniform(-70, -35)), ch, seed))
        else:
            parts.append(square(ms, rate, int(rng.choice([t1, t1 + 1, t2, t2 + 1, te, te + 1])), ch))
        total += ms
    x = cat(*parts)
    return x[:len(x) - int(rng.integers(0, 30))], rate, bool(rng.integers(0, 4))
