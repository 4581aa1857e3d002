"""One harness for "the same bits on a caller's side stream, behind a late producer" (tests/test_gpu_streams.py).

Every function of the C ABI takes a stream, and under pytest every call site hands it the legacy default stream.  `same_bits_on_a_side_stream`
runs a call there first (twice: run-to-run bit stability is established, not assumed) and then on a fresh `torch.cuda.Stream()`, where
the call's data inputs hold poison -- NaN for floats, 0x5555 for int16 PCM, 0x55 for bytes -- when the call is ISSUED: the real data is
copied in by the same stream behind a delay (a chain of dependent matmuls) that is sized per case to at least ten times the host time of the
default-stream call and never below 10 ms.  A kernel, memset or staged copy that went to another stream, or a host wait on another stream in
front of a read-back, reads the poison or an unwritten output; stream order on the one right stream never does.  Only values that kernels
treat as data are poisoned: lengths, offsets, indices and token ids are the caller's closed-over arguments and are complete before the
delay starts.

A case is three callables:
    inputs()            -> {name: device tensor}, the real data inputs, built on the default stream
    fresh()             -> whatever `run` needs beside them (a new handle, say); None where the entry has no handle
    run(ctx, tensors)   -> the outputs as a list of device tensors; `tensors` has the shapes and dtypes of inputs() and may be written to
"""
import math
import time

import torch

MIN_DELAY_MS = 10.0
DELAY_FACTOR = 10.0
_N = 2048                      # the delay's matmul: [_N, _N] fp32 by an orthogonal matrix, so the chain stays finite however long it is
_state = {}
REPORT = []                    # (case, host ms, delay ms) of every side-stream run of the process


def poison_like(t):
    if t.is_floating_point():
        return torch.full_like(t, float("nan"))
    if t.dtype == torch.int16:
        return torch.full_like(t, 0x5555)
    if t.dtype == torch.uint8:
        return torch.full_like(t, 0x55)
    raise TypeError(f"no poison for {t.dtype}: only values that kernels treat as data are poisoned")


def _delay_state():
    """The orthogonal matrix, the running product and the measured time of one link of the chain (events, default stream); once a process"""
    if not _state:
        g = torch.Generator().manual_seed(77)
        q, _ = torch.linalg.qr(torch.randn(_N, _N, generator=g, dtype=torch.float64))
        _state["q"] = q.float().cuda()
        _state["x"] = torch.eye(_N, device="cuda")
        for _ in range(20):
            _state["x"] = _state["x"] @ _state["q"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            _state["x"] = _state["x"] @ _state["q"]
        e1.record()
        torch.cuda.synchronize()
        _state["link_ms"] = e0.elapsed_time(e1) / 50
    return _state


def queue_delay(stream, want_ms):
    """Queues at least `want_ms` of dependent matmuls on `stream` (the current stream) -> (start event, end event) for the measurement"""
    st = _delay_state()
    links = max(int(math.ceil(1.5 * want_ms / st["link_ms"])), 4)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    x = st["q"]                                                    # (every product is allocated on `stream`; q is never freed)
    e0.record(stream)
    for _ in range(links):
        x = x @ st["q"]
    e1.record(stream)
    return e0, e1


def same(got, want, tag):
    """Bit equality of two lists of tensors; bytes and int16 by their bytes"""
    assert len(got) == len(want), f"{tag}: {len(got)} outputs vs {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{tag}: output {i} is {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
        if a.dtype in (torch.int16, torch.uint8):
            ok = a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        else:
            ok = torch.equal(a, b)
        if not ok:
            bad = a != b
            if a.is_floating_point():
                bad |= torch.isnan(a) | torch.isnan(b)
            first = int(bad.reshape(-1).nonzero()[0]) if bad.any() else -1
            nan = int(torch.isnan(a).sum()) if a.is_floating_point() else 0
            raise AssertionError(f"{tag}: output {i} differs in {int(bad.sum())} of {a.numel()} values (first at {first}), {nan} NaN")


def default_stream_run(name, inputs, fresh, run, stable=None):
    """The call on the default stream, twice on one context -> (want, real inputs, host ms of the first call).  The two results are
    bit-equal (`stable`: a comparison fn(got, want, tag) at the entry's existing tolerance, for an entry found not to be bit-stable)."""
    assert torch.cuda.current_stream().cuda_stream == 0, "the reference run is on the legacy default stream"
    real = inputs()
    torch.cuda.synchronize()
    ctx = fresh()
    work = {k: v.clone() for k, v in real.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(ctx, work)
    host_ms = (time.perf_counter() - t0) * 1e3
    want = [o.clone() for o in out]
    torch.cuda.synchronize()
    again = [o.clone() for o in run(ctx, {k: v.clone() for k, v in real.items()})]
    torch.cuda.synchronize()
    (stable or same)(again, want, f"{name}: second run on the default stream vs the first")
    return want, real, host_ms


def side_stream_run(name, real, ctx, run, host_ms, stream=None):
    """The call on a fresh side stream behind the late producer -> (outputs cloned on that stream, delay ms).  `real` are finished device
    tensors (the caller synchronised); the call is issued while `produced` has not happened."""
    s = torch.cuda.Stream() if stream is None else stream
    want_ms = max(DELAY_FACTOR * host_ms, MIN_DELAY_MS)
    with torch.cuda.stream(s):
        bufs = {k: poison_like(v) for k, v in real.items()}
        s.synchronize()                                            # the poison is there before the delay starts
        e0, e1 = queue_delay(s, want_ms)
        for k, v in real.items():
            bufs[k].copy_(v)
        produced = torch.cuda.Event()
        produced.record(s)
        assert not produced.query(), f"{name}: the inputs were already there when the call was issued"
        out = run(ctx, bufs)
        got = [o.clone() for o in out]
    s.synchronize()
    delay_ms = e0.elapsed_time(e1)
    REPORT.append((name, host_ms, delay_ms))
    print(f"[streams] {name}: host {host_ms:.3f} ms, delay {delay_ms:.1f} ms")
    assert delay_ms >= want_ms, f"{name}: the delay was {delay_ms:.2f} ms, below {want_ms:.2f} ms (10 x the host time, at least 10 ms)"
    return got, delay_ms


def same_bits_on_a_side_stream(name, inputs, fresh, run, stable=None, twice=True):
    """Default stream (twice), then a fresh context whose first call ever is on a fresh side stream behind the late producer, then (`twice`)
    the same context once more on another fresh side stream: every result bit-equal to the default stream's.  Returns the side-stream
    context for the caller's own checks (counters, say)."""
    want, real, host_ms = default_stream_run(name, inputs, fresh, run, stable)
    ctx = fresh()
    torch.cuda.synchronize()
    cmp = stable or same
    got, _ = side_stream_run(name + " [first call of its context]", real, ctx, run, host_ms)
    cmp(got, want, f"{name}: side stream vs the default stream")
    if twice:
        got, _ = side_stream_run(name + " [second call]", real, ctx, run, host_ms)
        cmp(got, want, f"{name}: side stream, second call on the context, vs the default stream")
    return ctx
