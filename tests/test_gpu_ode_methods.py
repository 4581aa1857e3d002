"""GPU: one ODE method per unit in one sampler call (f5hip_cfm_sample_methods, torch.ops.f5hip.cfm_sample_methods, `ode_method=` of
F5HipModel.sample / sample_units / plan_unit).  A unit stepped by its own solver inside a mixed-method call equals the same unit sampled
alone, through the one-method path, on a handle built with that solver, bit for bit (shape-invariant attention), for DiT, UNetT and MMDiT,
whole grids and spans, and stays within north_star's 1e-3 RMS of the CPU oracle's sampler; units whose forwards are done stop costing
backbone rows ("dit_rows"); the per-unit instance of cfg_step_kernel alone against fp64 and against the one-op instance; the serving manager samples requests
of different solvers in one call."""
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
from row_ops_ref import cfg_velocity, euler_step, fmt_split, rk4_stage, rk4_stage_abs  # noqa: E402
from test_gpu_request_knobs import ARCH, REF_TEXT, TINY, VOCAB, _backbone, _prompt, _rms, _units  # noqa: E402
from tts_indic_server_f5_amd import _lib, serve, synth, torch_ops  # noqa: E402

METHODS, STEPS = ["euler", "rk4", "midpoint", "rk4"], [6, 2, 3, 1]      # 6 / 8 / 6 / 4 forwards: three leaving points, one tie
CFGS, SWAYS = [2.0, 0.0, 3.5, 2.0], [-1.0, None, 0.5, -1.0]
FORWARDS = {"euler": 1, "midpoint": 2, "rk4": 4}
CODE = {"euler": 0, "midpoint": 1, "rk4": 2}


def _sample(model, units, cfg, steps, sway, **kw):
    conds = torch.nn.utils.rnn.pad_sequence([c[0] for c, _, _, _ in units], batch_first=True)
    texts = torch.nn.utils.rnn.pad_sequence([t[0] for _, t, _, _ in units], batch_first=True, padding_value=-1)
    lens = torch.tensor([c.shape[1] for c, _, _, _ in units])
    frames = torch.tensor([f for _, _, f, _ in units])
    out, _ = model.sample(conds, texts, frames, lens=lens, y0=[y for _, _, _, y in units], steps=steps, cfg_strength=cfg,
                          sway_sampling_coef=sway, **kw)
    return [out[i, :y.shape[0]] for i, (_, _, _, y) in enumerate(units)]


def _counter(name):
    v = C.c_int64()
    _lib.check(_lib.lib().f5hip_get_counter(name.encode(), C.byref(v)), "get_counter")
    return v.value


def _reset():
    _lib.check(_lib.lib().f5hip_get_counter(b"reset", None), "reset counters")


class _Handles:
    """One handle per solver of a backbone, built on first use: `alone(i, ...)` is unit i through the existing one-method path -- no
    `ode_method` argument, a handle built with odeint_kwargs=dict(method=...) -- and the yardstick of this file."""

    def __init__(self, kind):
        from tts_indic_server_f5_amd.model import F5HipModel
        self.arch, self.sd, self.fwd, self.cfg = _backbone(kind)
        self._make = lambda method: F5HipModel(self.arch, self.sd, odeint_kwargs=dict(method=method))
        self._by_method = {}

    def __getitem__(self, method):
        if method not in self._by_method:
            self._by_method[method] = self._make(method)
        return self._by_method[method]

    def alone(self, unit, method, steps, cfg, sway):
        return _sample(self[method], [unit], cfg, steps, sway)[0]

    def oracle(self, unit, method, steps, cfg, sway):
        cond, text, f, y0 = unit
        kw = dict(steps=steps, cfg_strength=cfg, sway_sampling_coef=sway, y0=y0[None], forward_fn=self.fwd)
        if method == "rk4":
            return cfm_sample_rk4(self.sd, self.cfg, cond, text, f, **kw)
        return O.cfm_sample(self.sd, self.cfg, cond, text, f, method=method, keep_trajectory=False, **kw)[0]


def _check_units(h, kind, units, mixed, methods, steps, cfgs, sways):
    for i, u in enumerate(units):
        alone = h.alone(u, methods[i], steps[i], cfgs[i], sways[i])
        diff = (mixed[i] - alone).abs().max().item()
        assert torch.equal(mixed[i], alone), f"{kind} unit {i} ({methods[i]}, {steps[i]} steps): max diff vs alone {diff:.3e}"
        p = u[0].shape[1]
        rms = _rms(mixed[i][p:], h.oracle(u, methods[i], steps[i], cfgs[i], sways[i])[0, p:])
        print(f"[parity] {kind} unit {i} ({methods[i]}, steps {steps[i]}, sway {sways[i]}, cfg {cfgs[i]}): rms vs oracle {rms:.3e}")
        assert rms < 1e-3


@pytest.mark.parametrize("kind", ["dit", "unett", "mmdit"])
def test_mixed_method_units_equal_alone_and_oracle(kind, attn_shape_invariant):
    h = _Handles(kind)
    units = _units()
    mixed = _sample(h["euler"], units, CFGS, STEPS, SWAYS, ode_method=METHODS)
    _check_units(h, kind, units, mixed, METHODS, STEPS, CFGS, SWAYS)
    assert h["euler"].ode_method == "euler"      # the handle's own method is left as it was: the next plain call is a Euler call
    again = _sample(h["euler"], units[:1], CFGS[0], STEPS[0], SWAYS[0])[0]
    assert torch.equal(again, mixed[0])


@pytest.mark.parametrize("kind", ["dit", "unett", "mmdit"])
def test_equal_forwards_nobody_leaves(kind, attn_shape_invariant):
    """Euler 4 steps, midpoint 2, RK4 1: four forwards each."""
    h = _Handles(kind)
    units = _units()[:3]
    methods, steps = ["euler", "midpoint", "rk4"], [4, 2, 1]
    mixed = _sample(h["euler"], units, CFGS[:3], steps, SWAYS[:3], ode_method=methods)
    _check_units(h, kind, units, mixed, methods, steps, CFGS[:3], SWAYS[:3])


def test_all_equal_list_is_the_one_method_call(attn_shape_invariant):
    h = _Handles("dit")
    units = _units()
    _reset()
    want = _sample(h["rk4"], units, CFGS, STEPS, SWAYS)
    rows = _counter("dit_rows")
    _reset()
    got = _sample(h["euler"], units, CFGS, STEPS, SWAYS, ode_method=["rk4"] * 4)
    assert _counter("dit_rows") == rows
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    for a, b in zip(_sample(h["euler"], units, CFGS, STEPS, SWAYS, ode_method="rk4"), want):      # one name for all items
        assert torch.equal(a, b)
    for a, b in zip(_sample(h["rk4"], units, CFGS, STEPS, SWAYS, ode_method=[None, "rk4", None, "rk4"]), want):   # None: the handle's
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["dit", "unett"])
def test_finished_units_cost_no_rows(kind, attn_shape_invariant):
    h = _Handles(kind)
    units = _units()
    extra = 1 if kind == "unett" else 0
    rows = [(-(-(y.shape[0] + extra) // 128) * 128) * (2 if c >= 1e-5 else 1) for (_, _, _, y), c in zip(units, CFGS)]
    fw = [s * FORWARDS[m] for s, m in zip(STEPS, METHODS)]
    _reset()
    _sample(h["euler"], units, CFGS, STEPS, SWAYS, ode_method=METHODS)
    got = _counter("dit_rows")
    expect = sum(r for f in range(max(fw)) for r, n in zip(rows, fw) if n > f)
    print(f"[rows] {kind} mixed methods: dit_rows {got}, all rows every forward {max(fw) * sum(rows)}")
    assert got == expect and got < max(fw) * sum(rows)


@pytest.mark.parametrize("kind", ["dit", "unett", "mmdit"])
def test_mixed_method_spans_equal_alone(kind, attn_shape_invariant):
    """advance(units, 2) on a Euler handle: 2 steps per span for the Euler unit, max(1, 2 * 1 // 2) = 1 for the midpoint unit and
    max(1, 2 * 1 // 4) = 1 for the RK4 units; the last unit is admitted one span late."""
    h = _Handles(kind)
    model, units = h["euler"], _units()
    planned = [model.plan_unit(c, t[0], f, steps=s, cfg_strength=g, sway_sampling_coef=w, y0=y, ode_method=m)
               for (c, t, f, y), s, g, w, m in zip(units, STEPS, CFGS, SWAYS, METHODS)]
    assert [p.method for p in planned] == METHODS
    cursors = lambda: [p.cursor for p in planned]
    assert model.advance(planned[:3], 2) == [] and cursors() == [2, 1, 1, 0]
    assert model.advance(planned, 2) == [planned[1], planned[3]] and cursors() == [4, 2, 2, 1]
    assert model.advance([planned[0], planned[2]], 2) == [planned[0], planned[2]] and cursors() == [6, 2, 3, 1]
    for i, (p, u) in enumerate(zip(planned, units)):
        alone = h.alone(u, METHODS[i], STEPS[i], CFGS[i], SWAYS[i])
        diff = (p.mel - alone).abs().max().item()
        print(f"[spans] {kind} unit {i} ({METHODS[i]}, steps {STEPS[i]}): max diff vs alone in one call {diff:.3e}")
        assert torch.equal(p.mel, alone), f"{kind} unit {i}: max diff {diff:.3e}"
    # a unit whose solver is the handle's takes max_steps, like a unit without one: the span is the plain span call
    c, t, f, y = units[0]
    own = model.plan_unit(c, t[0], f, steps=6, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y, ode_method="euler")
    plain = model.plan_unit(c, t[0], f, steps=6, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y)
    for span in (4, 4):
        model.advance([own], span)
        model.advance([plain], span)
        assert own.cursor == plain.cursor
    assert own.done and torch.equal(own.mel, plain.mel)


def _method_args(units, steps, sways, cfgs, methods):
    """The packed arguments of one cfm_sample_methods call for `units` (batch-1 semantics, no padding)."""
    from tts_indic_server_f5_amd.model import time_grid
    dur = [y.shape[0] for _, _, _, y in units]
    conds, masks = [], []
    for (c, t, f, y), d in zip(units, dur):
        conds.append(torch.nn.functional.pad(c[0], (0, 0, 0, d - c.shape[1])))
        masks.append(torch.arange(d) < c.shape[1])
    nt = max(t.shape[1] for _, t, _, _ in units)
    text = torch.full((len(units), nt), -1, dtype=torch.int32)
    for i, (_, t, _, _) in enumerate(units):
        text[i, :t.shape[1]] = t[0]
    grids = [time_grid(s, w) for s, w in zip(steps, sways)]
    return (torch.tensor(dur, dtype=torch.int32), torch.cat(conds).cuda().contiguous(), torch.cat(masks).to(torch.uint8), text,
            torch.cat([y for _, _, _, y in units]).cuda().contiguous(), torch.tensor(steps, dtype=torch.int32), torch.cat(grids),
            torch.tensor(cfgs, dtype=torch.float32), torch.tensor([CODE[m] for m in methods], dtype=torch.int32))


def test_cfm_sample_methods_torch_op_equals_ctypes_and_checks_arguments(attn_shape_invariant):
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    assert torch_ops.load()
    model = F5HipModel(DiTArch(**TINY), synth.dit_state_dict(**TINY))
    units = _units(seed=6)
    dur, cond, mask, text, y0, steps, tg, cfg, meth = _method_args(units, STEPS, SWAYS, CFGS, METHODS)
    op = torch_ops.ops().cfm_sample_methods
    via_op = op(int(model._h), dur, None, cond, mask, text, y0, steps, tg, cfg, meth, None)
    out = torch.empty_like(y0)
    l, P = _lib.lib(), (lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    args = lambda st, g, me, n=len(units): (model._h, n, P(dur), None, P(cond), P(mask), P(text), text.shape[1], P(y0), P(st), P(g), P(cfg), P(me), None,
                                            P(out), _lib.current_stream_ptr())
    _lib.check(l.f5hip_cfm_sample_methods(*args(steps, tg, meth)), "f5hip_cfm_sample_methods")
    torch.cuda.synchronize()
    assert torch.equal(via_op, out)
    # the model's path is the same call; `last` all 1 is `last` null
    for a, (i, b) in zip(_sample(model, units, CFGS, STEPS, SWAYS, ode_method=METHODS), enumerate(np.cumsum([0] + dur.tolist())[:-1])):
        assert torch.equal(a, via_op[b:b + dur[i]])
    assert torch.equal(op(int(model._h), dur, None, cond, mask, text, y0, steps, tg, cfg, meth, torch.ones(4, dtype=torch.uint8)), via_op)

    # refusals: by the operator and by the C entry point, before anything is launched
    def refused(call, match, c_args=None, c_match=None):
        _reset()
        with pytest.raises(RuntimeError, match=match):
            call()
        if c_args is not None:
            assert l.f5hip_cfm_sample_methods(*c_args) != 0 and c_match in l.f5hip_last_error(), l.f5hip_last_error()
        torch.cuda.synchronize()
        assert _counter("dit_rows") == 0

    _reset()
    assert l.f5hip_cfm_sample_methods(*args(steps, tg, None)) != 0 and b"method is null" in l.f5hip_last_error()
    assert _counter("dit_rows") == 0
    three = meth.clone(); three[2] = 3
    refused(lambda: op(int(model._h), dur, None, cond, mask, text, y0, steps, tg, cfg, three, None), "method\\[2\\] = 3", args(steps, tg, three), b"method[2] = 3")
    refused(lambda: op(int(model._h), dur, None, cond, mask, text, y0, steps, tg, cfg, meth[:3].contiguous(), None), "method needs one value per unit")
    zero = steps.clone(); zero[1] = 0
    refused(lambda: op(int(model._h), dur, None, cond, mask, text, y0, zero, tg, cfg, meth, None), "need >= 1", args(zero, tg, meth), b"steps[1] = 0")
    # Euler 128 + midpoint 64 + RK4 42 steps on three different sways: 128 + 128 + 127 points, far more than 256 distinct ones
    big_steps, big_methods = [128, 64, 42, 1], ["euler", "midpoint", "rk4", "rk4"]
    _, _, _, _, _, many, tg_many, _, meth_many = _method_args(units, big_steps, [-1.0, 0.5, None, -1.0], CFGS, big_methods)
    refused(lambda: op(int(model._h), dur, None, cond, mask, text, y0, many, tg_many, cfg, meth_many, None), "distinct time points",
            args(many, tg_many, meth_many), b"at most 256")
    # the handle is untouched: the same call again gives the same result
    _lib.check(l.f5hip_cfm_sample_methods(*args(steps, tg, meth)), "f5hip_cfm_sample_methods")
    torch.cuda.synchronize()
    assert torch.equal(via_op, out)


# ---------------------------------------------------------------------------------------------------------------- cfg_step_kernel<per unit> alone
DEV = "cuda"
MEL, ROWS = 100, 64
EPS16 = 16 * 2.0 ** -24           # tests/test_gpu_row_ops.py: at most 16 rounded fp32 operations, each relative to a partial sum bounded by S
XS_SENTINEL = -7.5                # exact in bf16: an untouched xs cell comes back as it went in
OPS = {"none": 0, "euler": 1, "half": 2, "full": 3, "rk1": 4, "rk2": 5, "rk3": 6, "rk4": 7}
# (frames per unit, op per unit, n_act).  13 frames each.  The issue asks for "13 frames over 5 units, one at a position >= n_act" AND "every
# op code present in one launch": eight op codes do not fit on four active units, so the first two cases are the 5-unit layout with the
# eight codes over two launches, and the third holds every code in ONE launch: eight active units (one of them "none") and one past n_act.
MIXED_CASES = {
    "5_units_a": ((3, 2, 4, 1, 3), ("euler", "half", "rk1", "rk2", "rk4"), 4),
    "5_units_b": ((3, 2, 4, 1, 3), ("full", "rk3", "rk4", "none", "euler"), 4),
    "every_op": ((2, 1, 2, 1, 2, 1, 2, 1, 1), ("rk2", "euler", "none", "half", "rk4", "full", "rk1", "rk3", "euler"), 8),
}
NO_UNCOND = 1                     # the unit without unconditional rows (strength 0)


def _mixed_layout(frames):
    urow_c, urow_u, funit, r0 = [], [], [], 0
    for k, n in enumerate(frames):
        urow_c += list(range(r0, r0 + n)); r0 += n + 1          # (one row between sequences belongs to no frame)
        if k == NO_UNCOND:
            urow_u += [-1] * n
        else:
            urow_u += list(range(r0, r0 + n)); r0 += n + 1
        funit += [k] * n
    assert r0 <= ROWS
    return np.array(urow_c, np.int32), np.array(urow_u, np.int32), np.array(funit, np.int32)


@pytest.mark.parametrize("case", list(MIXED_CASES))
def test_cfg_mixed_kernel_vs_fp64_and_one_method_kernels(case):
    """One launch of the per-unit instance of cfg_step_kernel through f5hip_op_cfg_mixed: every stepped element against the fp64 formulas of tests/row_ops_ref.py on
    the same fp32 inputs, |got - ref| <= 16 x 2^-24 x S (S: the absolute sum of the fp64 expression's terms; the bound derived in
    tests/test_gpu_row_ops.py), plus the split's 2^-16 |ref| where x_next exists only in xs; frames with op "none" or of a unit >= n_act,
    and every cell no frame owns, keep what they held; and per op code the frames are bit-equal to f5hip_op_cfg_step of that method /
    stage on the same inputs."""
    from tts_indic_server_f5_amd import ops
    frames, unit_ops, n_act = MIXED_CASES[case]
    n_units, U = len(frames), sum(frames)
    assert U == 13 and any(k >= n_act for k in range(n_units))
    urc, uru, funit = _mixed_layout(frames)
    g = torch.Generator().manual_seed(4242 + len(case))
    x0 = torch.randn(U, MEL, generator=g)
    pred = torch.randn(ROWS, 128, generator=g)
    k0 = [torch.randn(U, MEL, generator=g) for _ in range(3)]
    unit_cfg = [0.0 if k == NO_UNCOND else 1.0 + 0.37 * k for k in range(n_units)]
    unit_dt = [float(np.float32(0.021 + 0.013 * k)) for k in range(n_units)]
    fu = torch.from_numpy(funit).long()
    cfg_frame = torch.tensor(unit_cfg)[fu]
    d = lambda t: t.clone().to(DEV)
    x, xs, k = d(x0), torch.full((ROWS, 128), XS_SENTINEL, device=DEV), [d(t) for t in k0]
    ops.cfg_mixed(x, d(pred), urc, uru, xs, d(cfg_frame), funit, [OPS[o] for o in unit_ops], unit_dt, n_act, k)
    x, xs, k = x.cpu(), xs.cpu(), [t.cpu() for t in k]

    rc, has_u = torch.from_numpy(urc).long(), torch.from_numpy(uru >= 0)
    pc, pu = pred[rc, :MEL], pred[torch.from_numpy(np.maximum(uru, 0)).long(), :MEL]
    cfg64, dt64 = cfg_frame.double()[:, None], torch.tensor(unit_dt, dtype=torch.float64)[fu][:, None]
    v2, s2 = cfg_velocity(pc, pu, cfg64)
    v1, s1 = cfg_velocity(pc, None, cfg64)
    v, sv = torch.where(has_u[:, None], v2, v1), torch.where(has_u[:, None], s2, s1)
    xs_untouched = torch.ones(ROWS, 128, dtype=torch.bool)
    seen = set()
    for unit, op in enumerate(unit_ops):
        sel = fu == unit
        f_rc, f_ru = rc[sel], torch.from_numpy(uru).long()[sel]
        if unit >= n_act or op == "none":
            assert torch.equal(x[sel], x0[sel]) and all(torch.equal(a[sel], b[sel]) for a, b in zip(k, k0)), f"unit {unit} ({op}) was stepped"
            continue
        seen.add(op)
        xs_untouched[f_rc, :MEL] = False
        if unit != NO_UNCOND:
            xs_untouched[f_ru, :MEL] = False
            assert torch.equal(xs[f_rc, :MEL], xs[f_ru, :MEL]), f"unit {unit}: cond row != uncond row in xs"
        dt = dt64[sel]
        # the one-method kernel on the same inputs, per-unit-dt form with every unit active
        a, a_xs, a_k = d(x0), torch.full((ROWS, 128), XS_SENTINEL, device=DEV), [d(t) for t in k0]
        okw = dict(cfg_frame=d(cfg_frame), frame_unit=funit, unit_dt=unit_dt, n_act=n_units)
        if op in ("euler", "half", "full"):
            a_out = torch.full_like(a, 3.25) if op == "half" else a
            ops.cfg_step(ops.CFG_EULER, 0, a_out, a, d(pred), urc, uru, a_xs, **okw)
            out = k[0] if op == "half" else x          # the half step goes to the xmid / k1 rows of the frame, xstate untouched
            assert torch.equal(out[sel], a_out.cpu()[sel]), f"unit {unit} ({op}): not the Euler kernel's bits"
            ref, S = euler_step(x0[sel], v[sel], dt), x0[sel].double().abs() + dt * sv[sel]
            err = (out[sel].double() - ref).abs()
            assert (err <= EPS16 * S).all(), f"unit {unit} ({op}): max err / bound {(err / (EPS16 * S)).max().item():.3f}"
            assert torch.equal(xs[f_rc, :MEL], fmt_split(out[sel])), "xs != split(x_next)"
            if op == "half":
                assert torch.equal(x[sel], x0[sel]), "the half step changed xstate"
            assert all(torch.equal(k[j][sel], k0[j][sel]) for j in range(3) if not (op == "half" and j == 0))
        else:
            s = int(op[2])
            ops.cfg_step(ops.CFG_RK4, s - 1, None, a, d(pred), urc, uru, a_xs, k=a_k, **okw)
            assert torch.equal(x[sel], a.cpu()[sel]) and all(torch.equal(k[j][sel], a_k[j].cpu()[sel]) for j in range(3)), \
                f"unit {unit} ({op}): not the RK4 stage kernel's bits"
            ks = [t[sel] for t in k0[:s - 1]]
            ref, S = rk4_stage(s, x0[sel], v[sel], dt, *ks), rk4_stage_abs(s, x0[sel], sv[sel], dt, *ks)
            for j in range(3):
                if j == s - 1:
                    assert ((k[j][sel].double() - v[sel]).abs() <= EPS16 * sv[sel]).all(), f"k{s}"
                else:
                    assert torch.equal(k[j][sel], k0[j][sel]), f"stage {s} changed k{j + 1}"
            if s < 4:
                assert torch.equal(x[sel], x0[sel]), f"stage {s} changed xstate"
                assert ((xs[f_rc, :MEL].double() - ref).abs() <= EPS16 * S + 2.0 ** -16 * ref.abs()).all(), f"unit {unit} ({op}): xs out of bound"
            else:
                assert ((x[sel].double() - ref).abs() <= EPS16 * S).all(), f"unit {unit} ({op}): y1 out of bound"
                assert torch.equal(xs[f_rc, :MEL], fmt_split(x[sel])), "xs != split(y1)"
        assert torch.equal(xs[f_rc, :MEL], a_xs.cpu()[f_rc, :MEL]), f"unit {unit} ({op}): xs not the one-method kernel's bits"
    assert (xs[xs_untouched] == XS_SENTINEL).all(), "xs written outside the stepped frames' rows / past column 99"
    print(f"[parity] cfg_mixed {case}: ops stepped {sorted(seen)}")
    if case == "every_op":
        assert seen == set(OPS) - {"none"} and "none" in unit_ops[:n_act]


# ---------------------------------------------------------------------------------------------------------------- serving
def test_manager_two_ode_methods_one_sampler_call_equal_alone(tmp_path):
    """Two concurrent seeded requests, RK4 at 4 steps and Euler at 8, ride in one micro-batch and ONE sampler call; each equals the request
    served alone."""
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    from tts_indic_server_f5_amd.vocoder import F5HipVocos
    path = _prompt(tmp_path)
    model = F5HipModel(DiTArch(**ARCH), synth.dit_state_dict(**ARCH), vocab_char_map=VOCAB)
    calls, real = [], model.sample_units

    def counting(*a, **kw):
        calls.append(kw.get("ode_method"))
        return real(*a, **kw)

    model.sample_units = counting
    mgr = serve.TTSManager(nfe_step=8, micro_batch=dict(max_requests=8, max_wait_ms=300)).load(model, F5HipVocos(synth.vocos_state_dict()))
    reqs = [dict(text="Always remember, I am mighty and enduring.", ode_method="rk4", nfe_step=4, seed=21),
            dict(text="Respect me and I will nurture you.", ode_method="euler", nfe_step=8, seed=22)]
    try:
        mgr.synthesize("Warm up.", ref_audio_path=path, ref_text=REF_TEXT, seed=1)
        assert calls == [None]                   # a request without the option: the model is not handed it
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
        assert len(calls) == 1 and sorted(set(calls[0])) == ["euler", "rk4"], calls
        for i, r in enumerate(reqs):
            kw = dict(r)
            text = kw.pop("text")
            alone = mgr.synthesize(text, ref_audio_path=path, ref_text=REF_TEXT, **kw)
            np.testing.assert_array_equal(res[i], alone)
    finally:
        mgr.close()
