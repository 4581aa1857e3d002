"""The time tables of a handle (sinusoid, time MLP, AdaLN modulation; UNetT: the time token) are kept from one sampler call to the next
while the list of time points stays the same (csrc/f5hip.hip precompute_time; counter "time_table_builds").

Tiny DiT and UNetT: the same grid twice builds once and gives the same bits; steps 4 -> 5 -> 4 rebuilds every time, and every result equals
that of a fresh handle; a call with one grid per unit (f5hip_cfm_sample_grids: the union of the units' points) behaves the same way.
(Only the whole-grid sampler calls reuse: f5hip_cfm_sample_span and the single forward always build.)"""
import pytest
import torch

from test_gpu_request_knobs import CFGS, _backbone, _units
from test_gpu_time_grids import STEPS, SWAYS, _counter, _reset, _sample

pytestmark = pytest.mark.gpu


def _model(kind):
    from tts_indic_server_f5_amd.model import F5HipModel
    arch, sd, _, _ = _backbone(kind)
    return F5HipModel(arch, sd)


def _one_grid(model, units, steps):
    return torch.stack([o.clone() for o in _sample(model, units[:1], 2.0, steps, -1.0)])


@pytest.mark.parametrize("kind", ["dit", "unett"])
def test_same_grid_twice_builds_once(kind, attn_shape_invariant):
    model, units = _model(kind), _units()
    _reset()
    first = _one_grid(model, units, 4)
    assert _counter("time_table_builds") == 1
    second = _one_grid(model, units, 4)
    assert _counter("time_table_builds") == 1, "the second call on the same grid rebuilt the tables"
    assert torch.equal(first, second)


@pytest.mark.parametrize("kind", ["dit", "unett"])
def test_other_grid_in_between_rebuilds(kind, attn_shape_invariant):
    model, units = _model(kind), _units()
    fresh = {s: _one_grid(_model(kind), units, s) for s in (4, 5)}
    assert not torch.equal(fresh[4], fresh[5])
    _reset()
    for i, s in enumerate((4, 5, 4)):
        out = _one_grid(model, units, s)
        assert _counter("time_table_builds") == i + 1, f"call {i} (steps {s}) did not rebuild the tables"
        assert torch.equal(out, fresh[s]), f"call {i} (steps {s}) differs from a fresh handle"


@pytest.mark.parametrize("kind", ["dit", "unett"])
def test_per_unit_grids(kind, attn_shape_invariant):
    model, units = _model(kind), _units()
    other = [5, 3, 6, 4]
    fresh = {tuple(st): _sample(_model(kind), units, CFGS, st, SWAYS) for st in (STEPS, other)}
    _reset()
    first = _sample(model, units, CFGS, STEPS, SWAYS)
    assert _counter("time_table_builds") == 1
    second = _sample(model, units, CFGS, STEPS, SWAYS)
    assert _counter("time_table_builds") == 1, "the second call on the same grids rebuilt the tables"
    third = _sample(model, units, CFGS, other, SWAYS)
    assert _counter("time_table_builds") == 2
    fourth = _sample(model, units, CFGS, STEPS, SWAYS)
    assert _counter("time_table_builds") == 3
    for got, want in ((first, fresh[tuple(STEPS)]), (second, fresh[tuple(STEPS)]), (third, fresh[tuple(other)]), (fourth, fresh[tuple(STEPS)])):
        for a, b in zip(got, want):
            assert torch.equal(a, b)
