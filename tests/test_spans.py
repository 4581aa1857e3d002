"""Admission at span boundaries without a GPU: infer.SpanScheduler and serve.ContinuousBatcher over a fake model that implements
plan_unit / advance as fp32 Euler on a known vector field, through the host code the real model uses for its spans (model.time_grid,
model.span_slices, model.SpanUnit).  Order is driven by step() or by events, never by wall-clock time."""
import threading
from concurrent.futures import CancelledError

import numpy as np
import pytest
import torch

from tts_indic_server_f5_amd import infer, serve
from tts_indic_server_f5_amd.model import SpanUnit, span_slices, time_grid

MEL, HOP = 4, 256
WAIT = 60.0          # guard of every blocking wait: a broken batcher fails the test instead of hanging it


class SpanError(RuntimeError):
    pass


class BackendGone(RuntimeError):
    no_retry = True


def _field(t, x, cfg):
    return (cfg - x) * np.float32(t) + np.float32(0.25)


def _euler(noise, grid, cfg):
    x = noise.clone()
    for t0, t1 in zip(grid[:-1], grid[1:]):
        x = x + (t1 - t0) * _field(t0, x, np.float32(cfg))
    return x


class FakeModel:
    """plan_unit / advance as the real model offers them: noise drawn at planning, the grid built by model.time_grid, every span's steps and
    grid slices from model.span_slices."""
    resumable_spans = True

    def __init__(self):
        self.spans = []            # per advance call: [(unit, take, last, slice)]
        self.planned = []          # token lists, in planning order
        self.events = []
        self.error = None          # raised by a span that carries a unit whose text has a "#"
        self.entered, self.gate = threading.Event(), None

    def plan_unit(self, cond, tokens, frames, *, steps=32, cfg_strength=2.0, sway_sampling_coef=-1.0, generator=None, y0=None):
        if "!" in tokens:
            raise ValueError("cannot plan this text")
        noise = y0 if y0 is not None else torch.randn(int(frames), MEL, generator=generator)
        self.planned.append(list(tokens))
        self.events.append(("plan", "".join(tokens)))
        grid = np.ascontiguousarray(time_grid(int(steps), sway_sampling_coef).numpy().astype(np.float32))
        return SpanUnit(torch.zeros(int(frames), MEL), np.zeros(int(frames), np.uint8), list(tokens), grid, cfg_strength, noise)

    def advance(self, units, max_steps):
        take, last, tgs = span_slices(units, max_steps)
        self.events.append(("span", len(units)))
        self.entered.set()
        if self.gate is not None:
            assert self.gate.wait(WAIT)
        if self.error is not None and any("#" in u.text for u in units):
            raise self.error
        record, ended, o = [], [], 0
        for u, k, end in zip(units, take, last):
            sl = tgs[o:o + k + 1]
            o += k + 1
            u.state.copy_(_euler(u.state, sl, u.cfg_strength))
            record.append((u, k, int(end), sl.copy()))
            if u.stepped(k, end):
                ended.append(u)
        self.spans.append(record)
        return ended


class FakeVocoder:
    def decode(self, spec):            # [1, mel, T] -> [1, T * HOP]
        return spec.mean(dim=1).repeat_interleave(HOP, dim=1)


def _voice(seconds=1.0):
    wave = torch.sin(torch.arange(int(24000 * seconds), dtype=torch.float32) / 7.0)[None] * 0.2
    return infer.PreparedVoice((wave, 24000))


REF = "Hi there."


def _request(voice, text, **opts):
    return (voice, REF, text, opts) if opts else (voice, REF, text)


def _expected_waves(ticket, vocoder=FakeVocoder()):
    """The request's chunk waves from the noise its units drew, every unit sampled over its whole grid in one go."""
    mels = [_euler(u.noise, u.grid, u.cfg_strength) for u in ticket.units]
    (waves, _), = infer._chunk_waves([(mels, ticket.voice.ref_frames, ticket.voice.rms)], vocoder, "vocos", infer.target_rms)
    return waves


def _scheduler(model=None, **kw):
    model = model or FakeModel()
    return model, infer.SpanScheduler(model, FakeVocoder(), **kw)


def _reference_grid(n, sway):
    t = torch.linspace(0, 1, n + 1, dtype=torch.float32)          # cfm.py:196-198, as sample() writes it
    if sway is not None:
        t = t + sway * (torch.cos(torch.pi / 2 * t) - 1 + t)
    return t.numpy()


@pytest.mark.parametrize("sway", [-1.0, 0.5, None])
def test_span_slices_are_contiguous_bit_equal_slices_of_the_sample_grid(sway):
    voice = _voice()
    model, sched = _scheduler(span_steps=3, nfe_step=8, sway_sampling_coef=sway)
    nfe = [8, 5, 32, 3]
    tickets = [sched.admit(_request(voice, [f"Chunk {i}."], nfe_step=n) if n != 8 else _request(voice, [f"Chunk {i}."])) for i, n in enumerate(nfe)]
    done = []
    while sched.busy:
        done += sched.step()
    assert len(done) == 4 and all(t.done for t in tickets)
    for t, n in zip(tickets, nfe):
        unit, = t.units
        mine = [(k, last, sl) for span in model.spans for u, k, last, sl in span if u is unit]
        want = _reference_grid(n, sway)
        assert [k for k, _, _ in mine] == [3] * (n // 3) + ([n % 3] if n % 3 else [])        # min(span_steps, remaining)
        assert [last for _, last, _ in mine] == [0] * (len(mine) - 1) + [1]                 # `last` exactly once, at the end
        for (k, _, sl), (_, _, nxt) in zip(mine, mine[1:]):
            assert sl.dtype == np.float32 and len(sl) == k + 1 and sl[-1].tobytes() == nxt[0].tobytes()
        whole = np.concatenate([mine[0][2]] + [sl[1:] for _, _, sl in mine[1:]])
        assert whole.tobytes() == want.tobytes()
        np.testing.assert_array_equal(t.result[0], _expected_waves(t)[0])
    # a unit that ended mid-schedule left the spans: the 3-step request rode in one span only, the 32-step one ran on alone
    assert [len(s) for s in model.spans] == [4, 3, 2] + [1] * 8 and sched.span_units == [len(s) for s in model.spans]


def test_admission_order_max_frames_and_cancel():
    voice = _voice()
    model, sched = _scheduler(span_steps=2, nfe_step=4, max_frames=1000)
    a, b, c, d = [sched.admit(_request(voice, [text])) for text in ("A" * 40, "B" * 40, "C", "D")]
    frames = [t.frames for t in (a, b, c, d)]
    assert frames[0] + frames[1] <= 1000 < frames[0] + frames[1] + frames[2] and frames[2] == frames[3]
    assert sched.step() == [] and [t.in_flight for t in (a, b, c, d)] == [True, True, False, False]
    d.cancel()                                                 # waiting: never boards
    assert sched.step() == [a, b] and not c.in_flight          # c waited for room; nothing overtook it
    assert sched.step() == [] and c.in_flight and sched.waiting == []
    c.cancel()                                                 # in flight: leaves at the next boundary, half way
    assert sched.step() == [] and not sched.busy and c.units[0].cursor == 2 and not c.done
    assert sched.span_units == [2, 2, 1] and d.units[0].cursor == 0
    # arrival order is planning order, and a request larger than the cap runs when nothing else is in flight
    assert [p[-1] for p in model.planned] == ["A", "B", "C", "D"]
    big = sched.admit(_request(voice, ["E" * 400]))
    small = sched.admit(_request(voice, ["F"]))
    assert big.frames > 1000 and sched.step() == [] and big.in_flight and not small.in_flight
    assert sched.step() == [big] and sched.step() == [] and sched.step() == [small]


def test_unseeded_noise_is_drawn_at_admission_in_admission_order_and_seeded_from_its_own_generator():
    voice = _voice()
    _, sched = _scheduler(span_steps=2, nfe_step=4)
    torch.manual_seed(7)
    first = sched.admit(_request(voice, ["One.", "Two."]))
    seeded = sched.admit(_request(voice, ["Three.", "Four."], seed=3))
    second = sched.admit(_request(voice, ["Five."]))
    torch.manual_seed(7)
    for u in first.units + second.units:
        assert torch.equal(u.noise, torch.randn(u.dur, MEL))
    g = infer.request_generator(3)
    for u in seeded.units:
        assert torch.equal(u.noise, torch.randn(u.dur, MEL, generator=g))
    # a generator that continues a sequence moves only when the whole request was planned
    own = infer.request_generator(9)
    before = own.get_state()
    with pytest.raises(ValueError, match="cannot plan"):
        sched.admit(_request(voice, ["Fine.", "Not this one!"], generator=own))
    assert torch.equal(own.get_state(), before)
    ok = sched.admit(_request(voice, ["Fine."], generator=own))
    assert torch.equal(ok.units[0].noise, torch.randn(ok.units[0].dur, MEL, generator=infer.request_generator(9)))
    assert not torch.equal(own.get_state(), before)
    # a string is chunked and joined like infer_requests does; a list comes back chunk by chunk
    joined = sched.admit(_request(voice, "This is sentence one, quite long. And here is the second sentence, also long. A third one follows. " * 3, seed=1))
    while sched.busy:
        sched.step()
    assert len(joined.units) > 1 and joined.result.dtype == np.float32 and joined.result.ndim == 1
    np.testing.assert_array_equal(joined.result, np.asarray(infer.cross_fade_concat(_expected_waves(joined), infer.cross_fade_duration), np.float32))
    assert isinstance(first.result, list) and len(first.result) == 2


def _held_batcher(**kw):
    """A batcher whose worker cannot admit before the test lets go of the lock: what is submitted meanwhile is admitted together."""
    model, sched = _scheduler(**kw)
    lock = threading.Lock()
    lock.acquire()
    return model, sched, serve.ContinuousBatcher(sched, lock=lock), lock


def test_batcher_on_start_fires_at_admission_and_results_are_the_whole_grid_results():
    voice = _voice()
    model, sched, batcher, lock = _held_batcher(span_steps=2, nfe_step=4)
    futures = [batcher.submit(_request(voice, ["Head."]), on_start=lambda: model.events.append(("on_start", "head"))),
               batcher.submit(_request(voice, ["Other."]))]
    lock.release()
    waves = [f.result(timeout=WAIT) for f in futures]
    batcher.close()
    # admission = planning; the hook runs right behind it, before the request's first span
    assert model.events[:4] == [("plan", REF + " Head."), ("on_start", "head"), ("plan", REF + " Other."), ("span", 2)]
    assert batcher.batch_sizes == [2, 2] and len(waves[0]) == 1
    with pytest.raises(RuntimeError, match="closed"):
        batcher.submit(_request(voice, ["Late."]))


def test_batcher_cancel_while_queued_and_while_in_flight():
    voice = _voice()
    model, sched = _scheduler(span_steps=2, nfe_step=6)
    model.gate = threading.Event()
    batcher = serve.ContinuousBatcher(sched)
    a = batcher.submit(_request(voice, ["Goes away."]))
    assert model.entered.wait(WAIT)                 # a's first span is running; the worker is inside it
    b = batcher.submit(_request(voice, ["Never admitted."]))
    c = batcher.submit(_request(voice, ["Served."]))
    assert b.cancel() and a.cancel()                # queued / in flight
    model.gate.set()
    wave = c.result(timeout=WAIT)
    batcher.close()
    with pytest.raises(CancelledError):
        a.result(timeout=WAIT)
    assert [("".join(p)) for p in model.planned] == [REF + " Goes away.", REF + " Served."]
    first_unit = model.spans[0][0][0]
    assert first_unit.cursor == 2 and not first_unit.done          # it left at the boundary after the span it was in
    assert batcher.batch_sizes == [1, 1, 1, 1] and len(wave) == 1


def test_batcher_close_under_load_resolves_every_future():
    voice = _voice()
    model, sched, batcher, lock = _held_batcher(span_steps=3, nfe_step=8, max_frames=600)
    futures = [batcher.submit(_request(voice, [f"Request number {i}."], nfe_step=4 + i % 5)) for i in range(12)]
    closer = threading.Thread(target=batcher.close, kwargs=dict(timeout=WAIT))
    closer.start()
    lock.release()
    closer.join(WAIT)
    assert not closer.is_alive() and all(f.done() for f in futures)
    assert all(len(f.result()) == 1 for f in futures) and len(model.planned) == 12 and not sched.busy
    with pytest.raises(RuntimeError, match="closed"):
        batcher.submit(_request(voice, ["Late."]))


def test_raising_span_isolates_the_bad_request():
    voice = _voice()
    model, sched, batcher, lock = _held_batcher(span_steps=2, nfe_step=4)
    model.error = SpanError("bad unit")
    futures = [batcher.submit(_request(voice, [t], seed=i)) for i, t in enumerate(["Good one.", "Bad # one.", "Good two."])]
    lock.release()
    assert isinstance(futures[1].exception(timeout=WAIT), SpanError)
    for f, seed in ((futures[0], 0), (futures[2], 2)):
        got = f.result(timeout=WAIT)            # resolved: every span of its retry is in model.spans by now
        unit = next(u for span in model.spans for u, _, _, _ in span if torch.equal(u.noise, torch.randn(u.dur, MEL, generator=infer.request_generator(seed))))
        want = FakeVocoder().decode(_euler(unit.noise, unit.grid, unit.cfg_strength)[_voice().ref_frames:].t()[None]).squeeze().numpy()
        np.testing.assert_array_equal(got[0], want)         # from its first step, with the noise it already drew
    # one span with all three failed; then each request on its own: the good ones in two spans each, the bad one failing again
    assert [n for kind, n in model.events if kind == "span"] == [3, 1, 1, 1, 1, 1] and len(model.planned) == 3
    # a later request is served as usual
    assert len(batcher.submit(_request(voice, ["After."])).result(timeout=WAIT)) == 1
    batcher.close()


def test_no_retry_error_fails_every_request_in_flight_at_once():
    voice = _voice()
    model, sched, batcher, lock = _held_batcher(span_steps=2, nfe_step=4)
    model.error = BackendGone("a rank is down")
    futures = [batcher.submit(_request(voice, [t])) for t in ["Good one.", "Bad # one.", "Good two."]]
    lock.release()
    assert all(isinstance(f.exception(timeout=WAIT), BackendGone) for f in futures)
    assert [n for kind, n in model.events if kind == "span"] == [3] and not sched.busy
    batcher.close()


def test_a_request_that_cannot_be_planned_fails_alone():
    voice = _voice()
    model, sched, batcher, lock = _held_batcher(span_steps=2, nfe_step=4)
    futures = [batcher.submit(_request(voice, ["Fine."])), batcher.submit(_request(voice, ["Not this one!"])), batcher.submit(_request(voice, ["Fine too."]))]
    lock.release()
    assert isinstance(futures[1].exception(timeout=WAIT), ValueError)
    assert len(futures[0].result(timeout=WAIT)) == 1 and len(futures[2].result(timeout=WAIT)) == 1
    batcher.close()


def test_manager_selects_the_batcher_and_streams_head_and_tail_through_it():
    voice = _voice()
    model = FakeModel()
    mgr = serve.TTSManager(nfe_step=6, micro_batch=dict(span_steps=2, max_frames=4096, max_wait_ms=5)).load(model, FakeVocoder())
    try:
        assert isinstance(mgr.batcher, serve.ContinuousBatcher) and mgr.batcher.scheduler.span_steps == 2
        chunks = ["The head chunk.", "A tail chunk.", "Another tail chunk, a longer one."]
        pieces = list(mgr._stream(voice, REF, chunks[:1], chunks[1:], dict(generator=infer.request_generator(5))))
        g = infer.request_generator(5)
        waves = []
        for tokens in model.planned:
            unit = next(u for span in model.spans for u, _, _, _ in span if u.text == tokens)
            assert torch.equal(unit.noise, torch.randn(unit.dur, MEL, generator=g))             # head, then tail, one sequence
            waves.append(FakeVocoder().decode(_euler(unit.noise, unit.grid, 2.0)[voice.ref_frames:].t()[None]).squeeze().numpy())
        assert ["".join(p) for p in model.planned] == [REF + " " + c for c in chunks] and len(pieces) >= 2
        np.testing.assert_array_equal(np.concatenate(pieces), np.asarray(infer.cross_fade_concat(waves, infer.cross_fade_duration), np.float32))
        # the tail was admitted while the head was in flight: a span carried all three units
        assert 3 in mgr.batcher.batch_sizes
        # an edit takes the device lock between spans: the lock is free whenever no span runs
        assert mgr._device_lock.acquire(timeout=WAIT)
        mgr._device_lock.release()
    finally:
        mgr.close()
    assert mgr.batcher is None


def test_manager_without_span_steps_is_unchanged_and_refuses_models_without_spans():
    class Plain:
        def sample_units(self, *a, **kw):
            raise AssertionError("not called")

    mgr = serve.TTSManager(micro_batch=dict(max_requests=4, max_wait_ms=1)).load(Plain(), FakeVocoder())
    assert type(mgr.batcher) is serve.MicroBatcher
    mgr.close()
    assert serve.TTSManager().load(Plain(), FakeVocoder()).batcher is None
    with pytest.raises(ValueError, match="resumable spans"):
        serve.TTSManager(micro_batch=dict(span_steps=8)).load(Plain(), FakeVocoder())
    with pytest.raises(ValueError, match="resumable spans"):
        infer.SpanScheduler(Plain(), FakeVocoder(), span_steps=8)
    with pytest.raises(ValueError, match="span_steps"):
        infer.SpanScheduler(FakeModel(), FakeVocoder(), span_steps=0)
    # the measured default: the scheduler's own, and the manager's for dict(span_steps=None)
    assert infer.SpanScheduler(FakeModel(), FakeVocoder()).span_steps == infer.span_steps == 8
    mgr = serve.TTSManager(micro_batch=dict(span_steps=None, max_frames=4096)).load(FakeModel(), FakeVocoder())
    assert isinstance(mgr.batcher, serve.ContinuousBatcher) and mgr.batcher.scheduler.span_steps == infer.span_steps
    mgr.close()
