"""CPU: the pieces the host serving path shares -- `infer.plan_request` behind both `infer.infer_requests` and `infer.SpanScheduler.admit`
(option check, working copy of a caller's generator and its commit point), `infer.StreamJoiner.pieces`, and the queue / shutdown half
of `serve.MicroBatcher` and `serve.ContinuousBatcher` -- on stand-in model objects."""
import types

import numpy as np
import pytest
import torch

from tts_indic_server_f5_amd import infer, serve
from tts_indic_server_f5_amd.model import SpanUnit, time_grid

MEL = 4
REF = "Hi there."
CHUNKS = ["Chunk one.", "The second chunk is longer.", "Three."]


class SamplerFailed(RuntimeError):
    pass


class PlanModel:
    """Offers both `sample_units` and `plan_unit`: a unit's noise is `randn(frames, MEL)` from its generator, drawn unit by unit; the
    draw of unit `fail_at` raises instead."""
    resumable_spans = True

    def __init__(self, fail_at=None):
        self.fail_at, self.drawn = fail_at, 0

    def _draw(self, frames, generator):
        if self.drawn == self.fail_at:
            raise SamplerFailed("unit %d" % self.drawn)
        self.drawn += 1
        return torch.randn(int(frames), MEL, generator=generator)

    def sample_units(self, audio, units, *, steps, cfg_strength, sway_sampling_coef, generators=None):
        return [self._draw(frames, g) for (_, frames), g in zip(units, generators)]

    def plan_unit(self, cond, tokens, frames, *, steps=32, cfg_strength=2.0, sway_sampling_coef=-1.0, generator=None, y0=None):
        grid = np.ascontiguousarray(time_grid(int(steps), sway_sampling_coef).numpy().astype(np.float32))
        return SpanUnit(torch.zeros(int(frames), MEL), np.zeros(int(frames), np.uint8), list(tokens), grid, cfg_strength,
                        self._draw(frames, generator))


class Vocoder:
    def decode(self, spec):            # [1, mel, T] -> [1, T * 256]
        return spec.mean(dim=1).repeat_interleave(256, dim=1)


def _voice():
    wave = torch.sin(torch.arange(24000, dtype=torch.float32) / 7.0)[None] * 0.2
    return infer.PreparedVoice((wave, 24000))


def _run(path, model, request):
    if path == "infer_requests":
        return infer.infer_requests([request], model, Vocoder(), nfe_step=4)
    return infer.SpanScheduler(model, Vocoder(), nfe_step=4).admit(request)


@pytest.mark.parametrize("path", ["infer_requests", "admit"])
def test_a_callers_generator_moves_only_when_its_request_went_through(path):
    voice = _voice()
    _, units = infer._plan_request(voice, REF, CHUNKS, infer.target_rms, 1.0, None, None, infer.text_to_tokens)
    assert len(units) == 3 and len({frames for _, frames in units}) == 3
    start = torch.Generator().manual_seed(5).get_state()
    # the second chunk fails, after the first one drew from the working copy: the caller's generator has not moved
    gen = torch.Generator().manual_seed(5)
    with pytest.raises(SamplerFailed):
        _run(path, PlanModel(fail_at=1), (voice, REF, CHUNKS, dict(generator=gen)))
    assert torch.equal(gen.get_state(), start)
    # success: it stands where randn(dur_k, mel) for the chunks in order leaves it -- the same state on both paths
    model = PlanModel()
    _run(path, model, (voice, REF, CHUNKS, dict(generator=gen)))
    want = torch.Generator().manual_seed(5)
    for _, frames in units:
        torch.randn(frames, MEL, generator=want)
    assert model.drawn == 3 and torch.equal(gen.get_state(), want.get_state()) and not torch.equal(gen.get_state(), start)


def test_an_unknown_option_is_refused_with_one_message_on_both_paths():
    voice, texts = _voice(), []
    for path in ("infer_requests", "admit"):
        model = PlanModel()
        with pytest.raises(ValueError) as e:
            _run(path, model, (voice, REF, CHUNKS, dict(bogus=1, seed=3)))
        assert model.drawn == 0
        texts.append(str(e.value))
    assert texts[0] == texts[1] == f"unknown request option(s) ['bogus']; known: {list(infer.REQUEST_OPTIONS)}"


@pytest.mark.parametrize("fade_seconds", [0.15, 0.0])
def test_stream_joiner_pieces_are_the_non_empty_float32_pieces_of_the_joined_wave(fade_seconds):
    rng = np.random.default_rng(7)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (100, 5000, 3600, 1)]      # fade 0.15 s = 3600 samples
    joiner = infer.StreamJoiner(fade_seconds)
    pieces = list(joiner.pieces(waves[:2])) + list(joiner.pieces(waves[2:])) + list(joiner.pieces(flush=True))
    assert all(p.dtype == np.float32 and len(p) > 0 for p in pieces)
    assert np.array_equal(np.concatenate(pieces), np.asarray(infer.cross_fade_concat(waves, fade_seconds), np.float32))
    # 0.15 s: the first wave is held whole, the last two release nothing, the flush is the fade; 0 s: one piece per wave, nothing to flush
    assert [len(p) for p in pieces] == ([1400, 3600] if fade_seconds else [100, 5000, 3600, 1])
    assert list(joiner.pieces(flush=True)) == []        # nothing is held after the flush


BATCHERS = {"MicroBatcher": lambda: serve.MicroBatcher(lambda batch: batch, max_requests=2, max_wait_ms=1),
            "ContinuousBatcher": lambda: serve.ContinuousBatcher(types.SimpleNamespace(busy=False, span_units=[]))}


@pytest.mark.parametrize("kind", list(BATCHERS))
def test_a_closed_batcher_refuses_and_fails_what_is_left_under_its_own_name(kind):
    batcher = BATCHERS[kind]()
    name = type(batcher).__name__
    assert name == kind and batcher.batch_sizes == []
    batcher.close()
    assert not batcher._thread.is_alive()
    with pytest.raises(RuntimeError, match=f"^{name} is closed$"):
        batcher.submit("late")
    # a worker thread that is gone: a stranded item is failed, a cancelled one is left alone (no InvalidStateError)
    cancelled, stranded = serve.Future(), serve.Future()
    cancelled.cancel()
    batcher._q.put(("cancelled", cancelled, None))
    batcher._q.put(("stranded", stranded, None))
    batcher._fail_pending()
    assert cancelled.cancelled()
    with pytest.raises(RuntimeError, match=f"^{name} is closed$"):
        stranded.result(timeout=1)
