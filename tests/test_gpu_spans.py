"""GPU: resumable sampler spans (f5hip_cfm_sample_span, torch.ops.f5hip.cfm_sample_span, F5HipModel.plan_unit / advance) and admission at
span boundaries (infer.SpanScheduler, serve.ContinuousBatcher).  A unit sampled in spans of uneven length, with other units joining and
leaving between them, equals the same unit sampled alone in ONE cfm_sample_grids call, bit for bit (shape-invariant attention), for DiT,
UNetT and MMDiT under Euler, midpoint and RK4; a span over whole grids with `last` all 1 is f5hip_cfm_sample_grids, kernels and bits; at
F5-Base width the 32-step fixture unit in 4 spans of 8 equals the one-call result and stays within 1e-3 mel RMS of the reference's own
output; seeded requests admitted at different boundaries get the waves the plain serving path gives them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_request_knobs import ARCH, REF_TEXT, REQS, TEXT, TINY, VOCAB, _backbone, _prompt, _rms, _units  # noqa: E402
from test_gpu_time_grids import CFGS, STEPS, SWAYS, _grid_args  # noqa: E402
from tts_indic_server_f5_amd import _lib, infer, serve, synth, torch_ops  # noqa: E402

COUNTERS = ["gemm5_rb11", "gemm5_rb8", "gemm5_wide", "gemm5_cb12", "gemm3_wide", "gemm3", "conv5", "gemm6", "gemm6_r176", "gemm6_r256",
            "gemm_reg_bn64", "gemm_reg_bn128", "attn_bal8", "attn_nw8_deep", "attn_nw8", "attn_nw6_deep", "attn_nw6", "attn_nw4", "attn_seg2",
            "dit_rows"]


def _counters():
    out = {}
    for name in COUNTERS:
        v = C.c_int64()
        _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
        out[name] = v.value
    return out


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


def _alone(model, unit, steps, sway, cfg):
    """The unit alone in ONE cfm_sample_grids call."""
    dur, cond, mask, text, y0, st, tg, cf = _grid_args(model, [unit], [steps], [sway], [cfg])
    return torch_ops.ops().cfm_sample_grids(int(model._h), dur, None, cond, mask, text, y0, st, tg, cf)


def _plan(model, unit, steps, sway, cfg):
    cond, text, frames, y0 = unit
    return model.plan_unit(cond, text[0], frames, steps=steps, cfg_strength=cfg, sway_sampling_coef=sway, y0=y0)


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("kind", ["dit", "unett", "mmdit"])
def test_unit_in_uneven_spans_among_others_equals_alone(kind, method, attn_shape_invariant):
    """Unit 0 (6 steps) runs as spans of 3, 1 and 2 steps; units 1..3 (other voices, grids of 3 / 6 / 4 steps with other sways, CFG 0 / 3.5 /
    2) join before its second span and are gone before its last; they finish together afterwards, each at its own point of its grid."""
    from tts_indic_server_f5_amd.model import F5HipModel
    assert torch_ops.load()
    arch, sd, _, _ = _backbone(kind)
    model = F5HipModel(arch, sd, odeint_kwargs=dict(method=method))
    units = _units()
    planned = [_plan(model, u, s, w, c) for u, s, w, c in zip(units, STEPS, SWAYS, CFGS)]
    first, others = planned[0], planned[1:]
    assert model.advance([first], 3) == [] and first.cursor == 3 and not first.done
    assert model.advance([others[0], first, others[1], others[2]], 1) == [] and [p.cursor for p in planned] == [4, 1, 1, 1]
    assert model.advance([first], 5) == [first] and first.cursor == 6 and first.done
    ended = model.advance(others, 4)          # 2, 5 and 3 steps left: two of them end here
    assert ended == [others[0], others[2]] and others[1].remaining == 1
    assert model.advance([others[1]], 8) == [others[1]]
    for i, (p, u) in enumerate(zip(planned, units)):
        alone = _alone(model, u, STEPS[i], SWAYS[i], CFGS[i])
        diff = (p.mel - alone).abs().max().item()
        print(f"[spans] {kind} {method} unit {i} (steps {STEPS[i]}, sway {SWAYS[i]}, cfg {CFGS[i]}): max diff vs alone in one call {diff:.3e}")
        assert torch.equal(p.mel, alone), f"{kind} {method} unit {i}: max diff {diff:.3e}"
        n_prompt = u[0].shape[1]
        assert torch.equal(p.mel[:n_prompt].cpu(), u[0][0])      # the unit that ended got its prompt frames back (cfm.py:204)


@pytest.mark.parametrize("steps,sways", [(STEPS, SWAYS), ([6] * 4, [-1.0] * 4)], ids=["mixed_grids", "one_grid"])
def test_whole_grids_all_last_is_cfm_sample_grids(steps, sways, attn_shape_invariant):
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    assert torch_ops.load()
    model = F5HipModel(DiTArch(**TINY), synth.dit_state_dict(**TINY))
    dur, cond, mask, text, y0, st, tg, cfg = _grid_args(model, _units(seed=6), steps, sways, CFGS)
    _reset()
    grids = torch_ops.ops().cfm_sample_grids(int(model._h), dur, None, cond, mask, text, y0, st, tg, cfg)
    torch.cuda.synchronize()
    c_grids = _counters()
    _reset()
    span = torch_ops.ops().cfm_sample_span(int(model._h), dur, None, cond, mask, text, y0, st, tg, cfg, torch.ones(4, dtype=torch.uint8))
    torch.cuda.synchronize()
    c_span = _counters()
    print(f"[spans] counters grids {c_grids}\n[spans] counters span  {c_span}")
    assert torch.equal(span, grids)
    assert c_span == c_grids and c_grids["dit_rows"] > 0


def test_raw_state_of_a_unit_that_does_not_end(attn_shape_invariant):
    """`last` 0: all frames come back as the ODE state, prompt frames included (they differ from the conditioning); `last` 1: the same call's
    frames with the prompt overwritten.  Per unit, in one call."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    assert torch_ops.load()
    model = F5HipModel(DiTArch(**TINY), synth.dit_state_dict(**TINY))
    units = _units(seed=6)
    dur, cond, mask, text, y0, st, tg, cfg = _grid_args(model, units, STEPS, SWAYS, CFGS)
    run = lambda last: torch_ops.ops().cfm_sample_span(int(model._h), dur, None, cond, mask, text, y0, st, tg, cfg, torch.tensor(last, dtype=torch.uint8))
    ended, mixed, raw = run([1, 1, 1, 1]), run([1, 0, 0, 1]), run([0, 0, 0, 0])
    m, o = mask.bool().cuda(), 0
    for i, d in enumerate(dur.tolist()):
        sl = slice(o, o + d)
        assert torch.equal(mixed[sl], (ended if i in (0, 3) else raw)[sl])
        assert torch.equal(raw[sl][~m[sl]], ended[sl][~m[sl]])                 # generated frames: the same either way
        assert torch.equal(ended[sl][m[sl]], cond[sl][m[sl]]) and not torch.equal(raw[sl][m[sl]], cond[sl][m[sl]])
        o += d


def test_cfm_sample_span_torch_op_equals_ctypes_and_refuses_before_launch(attn_shape_invariant):
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    assert torch_ops.load()
    model = F5HipModel(DiTArch(**TINY), synth.dit_state_dict(**TINY))
    units = _units(seed=6)
    dur, cond, mask, text, y0, steps, tg, cfg = _grid_args(model, units, STEPS, SWAYS, CFGS)
    last = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)
    op = torch_ops.ops().cfm_sample_span
    via_op = op(int(model._h), dur, None, cond, mask, text, y0, steps, tg, cfg, last)
    out = torch.empty_like(y0)
    l, P = _lib.lib(), (lambda t: None if t is None else C.c_void_p(t.data_ptr()))

    def call(d=dur, kv=None, st=steps, g=tg, la=last):
        return l.f5hip_cfm_sample_span(model._h, len(units), P(d), P(kv), P(cond), P(mask), P(text), text.shape[1], P(y0), P(st), P(g), P(cfg), P(la),
                                       P(out), _lib.current_stream_ptr())

    _lib.check(call(), "f5hip_cfm_sample_span")
    torch.cuda.synchronize()
    assert torch.equal(via_op, out)
    # every refusal: by the operator and by the C entry point, with nothing launched (no backbone row was run)
    _reset()
    zero = steps.clone(); zero[1] = 0
    with pytest.raises(RuntimeError, match="need >= 1"):
        op(int(model._h), dur, None, cond, mask, text, y0, zero, tg, cfg, last)
    assert call(st=zero) != 0 and b"cfm_sample_span: steps[1] = 0" in l.f5hip_last_error()
    with pytest.raises(RuntimeError, match="sum\\(steps\\) \\+ n"):
        op(int(model._h), dur, None, cond, mask, text, y0, steps, tg[:-1], cfg, last)
    with pytest.raises(RuntimeError, match="last needs one value per unit"):
        op(int(model._h), dur, None, cond, mask, text, y0, steps, tg, cfg, last[:3])
    assert call(la=None) != 0 and b"last is null" in l.f5hip_last_error()
    bad_dur = dur.clone(); bad_dur[0] = 0; bad_dur[1] = dur[0] + dur[1]          # the same rows, unit 0 without any
    with pytest.raises(RuntimeError, match="dur\\[0\\] = 0 out of range"):
        op(int(model._h), bad_dur, None, cond, mask, text, y0, steps, tg, cfg, last)
    assert call(d=bad_dur) != 0 and b"dur[0] = 0 out of range" in l.f5hip_last_error()
    bad_kv = dur.clone(); bad_kv[2] += 1
    with pytest.raises(RuntimeError, match="kv_len\\[2\\]"):
        op(int(model._h), dur, bad_kv, cond, mask, text, y0, steps, tg, cfg, last)
    assert call(kv=bad_kv) != 0 and b"kv_len[2]" in l.f5hip_last_error()
    many = torch.tensor([200] * 4, dtype=torch.int32)                            # four distinct 200-step spans: ~800 time points
    _, _, _, _, _, _, tg_many, _ = _grid_args(model, units, [200] * 4, [-1.0, 0.0, 0.5, None], CFGS)
    with pytest.raises(RuntimeError, match="distinct time points"):
        op(int(model._h), dur, None, cond, mask, text, y0, many, tg_many, cfg, last)
    assert call(st=many, g=tg_many) != 0 and b"at most 256" in l.f5hip_last_error()
    one = torch.tensor([200] * 4, dtype=torch.int32)                             # one 200-step span for all: the one-grid limit
    tg_one = torch.linspace(0, 1, 201).repeat(4)
    with pytest.raises(RuntimeError, match="time points per call"):
        op(int(model._h), dur, None, cond, mask, text, y0, one, tg_one, cfg, last)
    assert _counters()["dit_rows"] == 0
    # the handle is untouched: the same call again gives the same result
    _lib.check(call(), "f5hip_cfm_sample_span")
    torch.cuda.synchronize()
    assert torch.equal(via_op, out)
    # the model's ctypes path is the same call
    planned = [_plan(model, u, s, w, c) for u, s, w, c in zip(units, STEPS, SWAYS, CFGS)]
    ctypes_planned = [_plan(model, u, s, w, c) for u, s, w, c in zip(units, STEPS, SWAYS, CFGS)]
    model.advance(planned, 2)
    load, torch_ops.load = torch_ops.load, (lambda: False)
    try:
        model.advance(ctypes_planned, 2)
    finally:
        torch_ops.load = load
    for a, b in zip(planned, ctypes_planned):
        assert torch.equal(a.state, b.state) and a.cursor == b.cursor == 2


def test_f5_base_width_four_spans_of_eight_equal_one_call_and_reference_digest(golden_dir):
    """F5-Base geometry, the 32-step fixture unit of tests/golden/cfm_base_sample_digest_s32.npz as 4 spans of 8; a second unit (another
    voice, 16 steps) is admitted after the first span and rides along for two spans."""
    from tts_indic_server_f5_amd.model import F5TTS_BASE, F5HipModel
    z = np.load(os.path.join(golden_dir, "cfm_base_sample_digest_s32.npz"))
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    model = F5HipModel(F5TTS_BASE, synth.dit_state_dict(), attn_shape_invariant=True)
    cond = torch.randn(1, 469, 100, generator=torch.Generator().manual_seed(14))
    kw = dict(steps=32, cfg_strength=2.0, sway_sampling_coef=-1.0)
    whole, _ = model.sample(cond, synth.text_ids(), 1404, seed=synth.SEED_NOISE, **kw)
    unit = model.plan_unit(cond, synth.text_ids()[0], 1404, generator=torch.Generator().manual_seed(synth.SEED_NOISE), **kw)
    g2 = torch.Generator().manual_seed(43)
    other = model.plan_unit(torch.randn(1, 300, 100, generator=g2), synth.text_ids(n_ref=40, n_gen=100)[0], 1380, steps=16, cfg_strength=2.0,
                            sway_sampling_coef=-1.0, generator=g2)
    assert model.advance([unit], 8) == []
    assert model.advance([unit, other], 8) == []
    assert model.advance([other, unit], 8) == [other]
    assert model.advance([unit], 8) == [unit]
    diff = (unit.mel - whole[0]).abs().max().item()
    got = unit.mel[469:].cpu().flatten()[g["idx"]]
    rms = _rms(got, g["sampled"])
    print(f"[spans] F5-Base 32 steps as 4 spans of 8: max diff vs one call {diff:.3e}; mel rms vs the reference digest {rms:.3e}")
    assert rms < 1e-3
    assert torch.equal(unit.mel[:4].cpu(), g["cond_head"])
    assert torch.equal(unit.mel, whole[0]), f"max diff {diff:.3e}"


def _manager(tmp_path, **micro_batch):
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    model = F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB)
    mgr = serve.TTSManager(nfe_step=8, micro_batch=micro_batch or None).load(model, F5HipVocos(synth.vocos_state_dict()))
    return mgr, _prompt(tmp_path)


def test_requests_admitted_at_different_boundaries_equal_the_plain_path(tmp_path):
    """A `SpanScheduler` over the manager's model, stepped here: three seeded requests (other speed, nfe_step, CFG strength, sway) are
    admitted before the first, the second and the third span; each wave equals `synthesize(..., seed=...)` of the plain path."""
    mgr, path = _manager(tmp_path)
    try:
        sched = infer.SpanScheduler(mgr.model_obj, mgr.vocoder, span_steps=3, **mgr.opts)
        voice, ref_text = mgr._voice(path, REF_TEXT)
        tickets, done = [], []
        for req in REQS:
            kw = dict(req)
            tickets.append(sched.admit((voice, ref_text, kw.pop("text"), kw)))
            done += sched.step()
        in_flight_at_admission = list(sched.span_units)
        while sched.busy:
            done += sched.step()
        print(f"[spans] units per span: {sched.span_units}")
        n = [len(t.units) for t in tickets]
        # the late requests joined while the first was in flight: the second span carries the first two requests' units, the third all
        assert in_flight_at_admission[:2] == [n[0], n[0] + n[1]] and sorted(map(id, done)) == sorted(map(id, tickets))
        for t, req in zip(tickets, REQS):
            kw = dict(req)
            plain = mgr.synthesize(kw.pop("text"), ref_audio_path=path, ref_text=REF_TEXT, **kw)
            np.testing.assert_array_equal(t.result, plain)
    finally:
        mgr.close()


def test_late_request_joins_through_the_manager_while_the_first_is_in_flight(tmp_path):
    """Through `TTSManager(span_steps=3)` and its `ContinuousBatcher`: the second request (6 steps) is submitted right after the first
    span of the first (8 steps) has run -- from a wrapper around the scheduler's `step`, so the order does not depend on timing -- and
    joins at the next boundary.  `batch_sizes` shows it, and both waves equal the plain path's."""
    mgr, path = _manager(tmp_path, span_steps=3)
    plain_mgr, _ = _manager(tmp_path)
    try:
        voice, ref_text = mgr._voice(path, REF_TEXT)
        reqs = []
        for r in REQS[:2]:
            kw = dict(r)
            reqs.append(mgr._request(voice, ref_text, kw.pop("text"), kw))
        n = [len(infer.request_chunks(ref_text, voice.seconds, r[2])) for r in reqs]
        sched, late = mgr.batcher.scheduler, []
        step = sched.step

        def step_then_submit():
            finished = step()
            if not late:
                late.append(mgr.batcher.submit(reqs[1]))
            return finished

        sched.step = step_then_submit
        first = mgr.batcher.submit(reqs[0]).result(timeout=120.0)
        second = late[0].result(timeout=120.0)
        print(f"[spans] units per span through the manager: {mgr.batcher.batch_sizes}; units per request {n}")
        assert mgr.batcher.batch_sizes == [n[0], n[0] + n[1], n[0] + n[1]]      # 8 steps in spans of 3; 6 steps in the last two of them
        for w, r in zip((first, second), REQS[:2]):
            kw = dict(r)
            np.testing.assert_array_equal(w, plain_mgr.synthesize(kw.pop("text"), ref_audio_path=path, ref_text=REF_TEXT, **kw))
    finally:
        mgr.close()
        plain_mgr.close()


def test_manager_with_span_steps_serves_and_streams_the_plain_waves(tmp_path):
    mgr, path = _manager(tmp_path, span_steps=3)
    plain_mgr, _ = _manager(tmp_path)
    try:
        assert isinstance(mgr.batcher, serve.ContinuousBatcher)
        kw = dict(REQS[0])
        text = kw.pop("text")
        plain = plain_mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, **kw)
        np.testing.assert_array_equal(mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, **kw), plain)
        assert len(mgr.batcher.batch_sizes) == 3                     # 8 steps in spans of 3
        pieces = list(mgr.synthesize_stream(text, ref_audio_path=path, ref_text=REF_TEXT, **kw))
        assert len(pieces) >= 2
        np.testing.assert_array_equal(np.concatenate(pieces), plain)
        assert TEXT == text
    finally:
        mgr.close()
        plain_mgr.close()
