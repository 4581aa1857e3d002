"""GPU: one time grid per unit in one sampler call (f5hip_cfm_sample_grids, torch.ops.f5hip.cfm_sample_grids).  A unit sampled inside a
mixed-grid call equals the same unit sampled alone with its grid as the call's, bit for bit (shape-invariant attention), for DiT, UNetT
and MMDiT under Euler, midpoint and RK4, and stays within north_star's 1e-3 RMS of the CPU oracle's sampler on that grid; units whose
steps are done stop costing backbone rows ("dit_rows"); the serving manager samples requests of different nfe_step in one call."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import dit_oracle as O  # noqa: E402
from rk4_oracle import cfm_sample_rk4  # noqa: E402
from test_gpu_request_knobs import ARCH, REF_TEXT, VOCAB, _backbone, _prompt, _rms, _units  # noqa: E402
from tts_indic_server_f5_amd import _lib, serve, synth, torch_ops  # noqa: E402

STEPS, SWAYS, CFGS = [6, 3, 6, 4], [-1.0, None, 0.5, -1.0], [2.0, 0.0, 3.5, 2.0]


def _sample(model, units, cfg, steps, sway):
    conds = torch.nn.utils.rnn.pad_sequence([c[0] for c, _, _, _ in units], batch_first=True)
    texts = torch.nn.utils.rnn.pad_sequence([t[0] for _, t, _, _ in units], batch_first=True, padding_value=-1)
    lens = torch.tensor([c.shape[1] for c, _, _, _ in units])
    frames = torch.tensor([f for _, _, f, _ in units])
    out, _ = model.sample(conds, texts, frames, lens=lens, y0=[y for _, _, _, y in units], steps=steps, cfg_strength=cfg,
                          sway_sampling_coef=sway)
    return [out[i, :y.shape[0]] for i, (_, _, _, y) in enumerate(units)]


def _counter(name):
    v = C.c_int64()
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("kind", ["dit", "unett", "mmdit"])
def test_mixed_grid_units_equal_alone_and_oracle(kind, method, attn_shape_invariant):
    from tts_indic_server_f5_amd.model import F5HipModel
    arch, sd, fwd, cfg = _backbone(kind)
    model = F5HipModel(arch, sd, odeint_kwargs=dict(method=method))
    units = _units()
    mixed = _sample(model, units, CFGS, STEPS, SWAYS)
    for i, u in enumerate(units):
        alone = _sample(model, [u], CFGS[i], STEPS[i], SWAYS[i])[0]
        assert torch.equal(mixed[i], alone), f"{kind} {method} unit {i}: max diff {(mixed[i] - alone).abs().max().item():.3e}"
        cond, text, f, y0 = u
        kw = dict(steps=STEPS[i], cfg_strength=CFGS[i], sway_sampling_coef=SWAYS[i], y0=y0[None], forward_fn=fwd)
        if method == "rk4":
            ref = cfm_sample_rk4(sd, cfg, cond, text, f, **kw)
        else:
            ref, _ = O.cfm_sample(sd, cfg, cond, text, f, method=method, keep_trajectory=False, **kw)
        p = cond.shape[1]
        rms = _rms(mixed[i][p:], ref[0, p:])
        print(f"[parity] {kind} {method} unit {i} (steps {STEPS[i]}, sway {SWAYS[i]}): rms vs oracle {rms:.3e}")
        assert rms < 1e-3
    # one grid for every unit, given as lists: the scalar call, bit for bit
    for a, b in zip(_sample(model, units, CFGS, [6] * 4, [-1.0] * 4), _sample(model, units, CFGS, 6, -1.0)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("method,per", [("euler", 1), ("rk4", 4)])
@pytest.mark.parametrize("kind", ["dit", "unett"])
def test_finished_units_cost_no_rows(kind, method, per, attn_shape_invariant):
    from tts_indic_server_f5_amd.model import F5HipModel
    arch, sd, _, _ = _backbone(kind)
    model = F5HipModel(arch, sd, odeint_kwargs=dict(method=method))
    units = _units()
    extra = 1 if kind == "unett" else 0
    rows = [(-(-(y.shape[0] + extra) // 128) * 128) * (2 if c >= 1e-5 else 1) for (_, _, _, y), c in zip(units, CFGS)]
    _reset()
    _sample(model, units, CFGS, STEPS, SWAYS)
    got = _counter("dit_rows")
    expect = per * sum(r for i in range(max(STEPS)) for r, s in zip(rows, STEPS) if s > i)
    print(f"[rows] {kind} {method}: dit_rows {got}, all rows every iteration {per * max(STEPS) * sum(rows)}")
    assert got == expect and got < per * max(STEPS) * sum(rows)


def test_f5_base_width_mixed_steps_vs_alone_and_oracle():
    """F5-Base geometry (real-width block GEMMs, default mixed mode): four units of ~1 400 frames at steps 8, 4, 8, 2 in one call."""
    from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel, unit_duration
    sd, cfg = synth.dit_state_dict(), O.DiTConfig()
    model = F5HipModel(F5TTS_BASE, sd, attn_shape_invariant=True)
    g = torch.Generator().manual_seed(41)
    units, steps = [], [8, 4, 8, 2]
    for p, n_gen, f in [(300, 120, 1400), (280, 100, 1380), (320, 110, 1420), (260, 90, 1360)]:
        cond = torch.randn(1, p, 100, generator=g)
        text = synth.text_ids(n_ref=40, n_gen=n_gen)
        units.append((cond, text, f, torch.randn(unit_duration(p, text.shape[1], f), 100, generator=g)))
    mixed = _sample(model, units, 2.0, steps, -1.0)
    for i, u in enumerate(units):
        alone = _sample(model, [u], 2.0, steps[i], -1.0)[0]
        diff = (mixed[i] - alone).abs().max().item()
        print(f"[alone] F5-Base unit {i} (steps {steps[i]}, {alone.shape[0]} frames): max diff vs alone {diff:.3e}")
        assert diff < 2e-5
        cond, text, f, y0 = u
        ref, _ = O.cfm_sample(sd, cfg, cond, text, f, steps=steps[i], cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0[None], keep_trajectory=False)
        p = cond.shape[1]
        rms = _rms(mixed[i][p:], ref[0, p:])
        print(f"[parity] F5-Base unit {i}: rms vs oracle {rms:.3e}")
        assert rms < 1e-3


def _grid_args(model, units, steps, sways, cfgs):
    """The packed arguments of one cfm_sample_grids call for `units` (batch-1 semantics, no padding)."""
    dur = [y.shape[0] for _, _, _, y in units]
    conds, masks = [], []
    for (c, t, f, y), d in zip(units, dur):
        conds.append(torch.nn.functional.pad(c[0], (0, 0, 0, d - c.shape[1])))
        masks.append(torch.arange(d) < c.shape[1])
    nt = max(t.shape[1] for _, t, _, _ in units)
    text = torch.full((len(units), nt), -1, dtype=torch.int32)
    for i, (_, t, _, _) in enumerate(units):
        text[i, :t.shape[1]] = t[0]
    grids = []
    for s, w in zip(steps, sways):
        t = torch.linspace(0, 1, s + 1, dtype=torch.float32)
        grids.append(t if w is None else t + w * (torch.cos(torch.pi / 2 * t) - 1 + t))
    return (torch.tensor(dur, dtype=torch.int32), torch.cat(conds).cuda().contiguous(), torch.cat(masks).to(torch.uint8), text,
            torch.cat([y for _, _, _, y in units]).cuda().contiguous(), torch.tensor(steps, dtype=torch.int32), torch.cat(grids),
            torch.tensor(cfgs, dtype=torch.float32))


def test_cfm_sample_grids_torch_op_equals_ctypes_and_checks_arguments(attn_shape_invariant):
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from test_gpu_request_knobs import TINY
    assert torch_ops.load()
    model = F5HipModel(DiTArch(**TINY), synth.dit_state_dict(**TINY))
    units = _units(seed=6)
    dur, cond, mask, text, y0, steps, tg, cfg = _grid_args(model, units, STEPS, SWAYS, CFGS)
    via_op = torch_ops.ops().cfm_sample_grids(int(model._h), dur, None, cond, mask, text, y0, steps, tg, cfg)
    out = torch.empty_like(y0)
    l, P = _lib.lib(), (lambda t: C.c_void_p(t.data_ptr()))
    args = lambda st, g: (model._h, len(units), P(dur), None, P(cond), P(mask), P(text), text.shape[1], P(y0), P(st), P(g), P(cfg), P(out),
                          _lib.current_stream_ptr())
    _lib.check(l.f5hip_cfm_sample_grids(*args(steps, tg)), "f5hip_cfm_sample_grids")
    torch.cuda.synchronize()
    assert torch.equal(via_op, out)
    # the model's path is the same call
    for a, (i, b) in zip(_sample(model, units, CFGS, STEPS, SWAYS), enumerate(np.cumsum([0] + dur.tolist())[:-1])):
        assert torch.equal(a, via_op[b:b + dur[i]])
    # bad arguments: refused by the op and by the C entry point, before anything is launched
    zero = steps.clone(); zero[1] = 0
    with pytest.raises(RuntimeError, match="need >= 1"):
        torch_ops.ops().cfm_sample_grids(int(model._h), dur, None, cond, mask, text, y0, zero, tg, cfg)
    with pytest.raises(RuntimeError, match="sum\\(steps\\) \\+ n"):
        torch_ops.ops().cfm_sample_grids(int(model._h), dur, None, cond, mask, text, y0, steps, tg[:-1], cfg)
    assert l.f5hip_cfm_sample_grids(*args(zero, tg)) != 0 and b"steps[1] = 0" in l.f5hip_last_error()
    many = torch.tensor([200, 200, 200, 200], dtype=torch.int32)   # four distinct 200-step Euler grids: ~800 time points
    _, _, _, _, _, _, tg_many, _ = _grid_args(model, units, [200] * 4, [-1.0, 0.0, 0.5, None], CFGS)
    with pytest.raises(RuntimeError, match="distinct time points"):
        torch_ops.ops().cfm_sample_grids(int(model._h), dur, None, cond, mask, text, y0, many, tg_many, cfg)
    assert l.f5hip_cfm_sample_grids(*args(many, tg_many)) != 0 and b"at most 256" in l.f5hip_last_error()
    # the handle is untouched: the same call again gives the same result
    _lib.check(l.f5hip_cfm_sample_grids(*args(steps, tg)), "f5hip_cfm_sample_grids")
    torch.cuda.synchronize()
    assert torch.equal(via_op, out)


def test_manager_two_nfe_steps_one_sampler_call_equal_alone(tmp_path):
    """Two concurrent seeded requests at nfe_step 16 and 32 ride in one micro-batch and ONE sampler call; each equals the request alone."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    path = _prompt(tmp_path)
    model = F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB)
    calls, real = [], model.sample_units

    def counting(*a, **kw):
        calls.append(kw.get("steps"))
        return real(*a, **kw)

    model.sample_units = counting
    mgr = serve.TTSManager(nfe_step=8, micro_batch=dict(max_requests=8, max_wait_ms=300)).load(model, F5HipVocos(synth.vocos_state_dict()))
    reqs = [dict(text="Always remember, I am mighty and enduring.", nfe_step=16, seed=21),
            dict(text="Respect me and I will nurture you.", nfe_step=32, seed=22)]
    try:
        mgr.synthesize("Warm up.", ref_audio_path=path, ref_text=REF_TEXT, seed=1)
        res, barrier = [None] * 2, threading.Barrier(2)

        def run(i):
            kw = dict(reqs[i])
            text = kw.pop("text")
            barrier.wait()
            res[i] = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, **kw)

        calls.clear()
        threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=600)
        assert mgr.batcher.batch_sizes[-1] == 2, mgr.batcher.batch_sizes
        assert len(calls) == 1 and sorted(set(calls[0])) == [16, 32], calls
        for i, r in enumerate(reqs):
            kw = dict(r)
            text = kw.pop("text")
            alone = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, **kw)
            np.testing.assert_array_equal(res[i], alone)
    finally:
        mgr.close()
