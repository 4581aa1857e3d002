"""CPU: the per-request `ode_method` option on stand-in samplers -- validation and the 400s of the three speech routes and the edit route,
the `nfe_step` limit that follows the request's solver, the option reaching the model object only for requests that set it (whole
calls, spans, sharded jobs, edits, a streamed request's tail), and the forwards budget of `model.span_slices`."""
import base64
import os
import sys
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tts_indic_server_f5_amd import infer, model as M, serve  # noqa: E402
from tts_indic_server_f5_amd.model import unit_duration  # noqa: E402

MSG = "ode_method must be one of 'euler', 'midpoint', 'rk4' (got "


class MethodModel:
    """`sample_units` / `plan_unit` / `advance` / `sample` of F5HipModel in closed form; every call's keyword arguments are recorded as they
    arrive, so a test sees whether `ode_method` was handed over at all."""
    device = torch.device("cpu")
    odeint_kwargs = dict(method="euler")
    resumable_spans = True
    per_unit_time_grids = True

    def __init__(self):
        self.calls, self.planned, self.spans, self.samples = [], [], [], []

    def cond_mel(self, audio):
        n = audio.shape[-1] // 256 + 1                                 # the frames of the real front-end (centred STFT, hop 256)
        return torch.nn.functional.pad(audio[0], (0, n * 256 - audio.shape[-1])).reshape(n, 256).mean(1, keepdim=True).repeat(1, 100)[None]

    def sample_units(self, audio, units, **kw):
        self.calls.append(dict(kw, n=len(units)))
        audios = list(audio) if isinstance(audio, (list, tuple)) else [audio] * len(units)
        out = []
        for a, (tokens, frames) in zip(audios, units):
            mel = self.cond_mel(a) if a.ndim == 2 else a
            dur = unit_duration(mel.shape[1], len(tokens), frames)
            out.append(torch.linspace(-1, 1, dur * 100).reshape(dur, 100))
        return out

    def plan_unit(self, cond, tokens, frames, **kw):
        self.planned.append(kw)
        dur = unit_duration(cond.shape[1], len(tokens), frames)
        return M.SpanUnit(cond[0], np.zeros(dur, np.uint8), np.zeros(len(tokens), np.int32), M.time_grid(int(kw["steps"]), None).numpy(),
                          kw["cfg_strength"], torch.zeros(dur, 100), method=kw.get("ode_method"))

    def advance(self, units, max_steps):
        take, last, _ = M.span_slices(units, max_steps, self.odeint_kwargs["method"])
        self.spans.append([(u.method, k) for u, k in zip(units, take)])
        return [u for u, k, end in zip(units, take, last) if u.stepped(k, end)]

    def sample(self, cond, text, duration, **kw):
        self.samples.append(kw)
        n = int(duration.max()) + 1 if isinstance(duration, torch.Tensor) else int(duration) + 1
        b = cond.shape[0]
        return torch.zeros(b, max(n, cond.shape[1] + 1), 100), None


class Vocoder:
    def decode(self, mel):
        t = mel.shape[-1]
        return (torch.sin(torch.arange(256 * (t - 1), dtype=torch.float32) * 0.01) * 0.1)[None]

    def decode_ragged(self, mels):
        return [self.decode(m[None])[0] for m in mels]


def _clip(freq, seconds=2.0, amp=0.3):
    return (amp * torch.sin(2 * torch.pi * freq * torch.arange(int(24000 * seconds)) / 24000))[None], 24000


REF_TEXT = "Hi there."
LONG = ("The quick brown fox jumps over the lazy dog. Pack my box with five dozen liquor jugs. How vexingly quick daft zebras jump. "
        "Sphinx of black quartz, judge my vow. The five boxing wizards jump quickly. Jackdaws love my big sphinx of quartz.")


# ------------------------------------------------------------------------------------------------------------------ validation
def test_check_request_options_validates_the_method_and_bounds_nfe_step_by_it():
    assert "ode_method" in infer.REQUEST_OPTIONS and "ode_method" in serve.EDIT_OPTIONS
    for name in ("euler", "midpoint", "rk4"):
        assert serve.check_request_options(dict(ode_method=name)) == dict(ode_method=name)
    assert serve.check_request_options(dict(ode_method=None, nfe_step=None)) == {}
    for bad in ("heun", "RK4", "", 2, True, ["rk4"]):
        with pytest.raises(ValueError) as e:
            serve.check_request_options(dict(ode_method=bad))
        assert str(e.value) == f"{MSG}{bad!r})"
    # the limit is the request's solver's when it names one (whatever the order of the fields), else the model's
    for opts in (dict(nfe_step=43, ode_method="rk4"), dict(ode_method="rk4", nfe_step=43)):
        with pytest.raises(ValueError, match="between 1 and 42 for the rk4 solver"):
            serve.check_request_options(opts, "euler")
    assert serve.check_request_options(dict(nfe_step=43, ode_method="euler"), "rk4") == dict(nfe_step=43, ode_method="euler")
    with pytest.raises(ValueError, match="between 1 and 42 for the rk4 solver"):
        serve.check_request_options(dict(nfe_step=43), "rk4")
    with pytest.raises(ValueError, match="between 1 and 64 for the midpoint solver"):
        serve.check_request_options(dict(nfe_step=65, ode_method="midpoint"), "euler")


def test_model_helpers_validate_names_and_lengths():
    assert M.per_unit_methods(None, 3) is None and M.per_unit_methods([None] * 3, 3) is None
    assert M.per_unit_methods("rk4", 2) == ["rk4", "rk4"] and M.per_unit_methods(["rk4", None], 2) == ["rk4", None]
    with pytest.raises(ValueError, match="one name per unit"):
        M.per_unit_methods(["rk4"], 2)
    with pytest.raises(ValueError, match="must be one of 'euler', 'midpoint', 'rk4'"):
        M.per_unit_methods(["rk4", "dopri5"], 2)


# ------------------------------------------------------------------------------------------------------------------ span budget
def _span_unit(steps, method=None):
    return M.SpanUnit(None, None, None, M.time_grid(steps, -1.0).numpy(), 2.0, torch.zeros(4, 100), method=method)


def test_span_slices_budgets_units_with_their_own_method_in_forwards():
    units = [_span_unit(6), _span_unit(6, "euler"), _span_unit(6, "midpoint"), _span_unit(6, "rk4")]
    for handle, max_steps, want in [("euler", 2, [2, 2, 1, 1]), ("euler", 4, [4, 4, 2, 1]), ("euler", 8, [6, 6, 4, 2]), ("rk4", 1, [1, 4, 2, 1]),
                                    ("rk4", 2, [2, 6, 4, 2]), ("midpoint", 3, [3, 6, 3, 1]), ("midpoint", 1, [1, 2, 1, 1])]:
        take, last, grids = M.span_slices(units, max_steps, handle)
        assert take == want, (handle, max_steps, take)
        assert list(last) == [int(k == 6) for k in take] and len(grids) == sum(take) + 4
    # without the handle's method the default is Euler's, and a unit without a method of its own is budgeted in steps as before
    assert M.span_slices(units[:1], 5)[0] == [5]
    u = _span_unit(3, "rk4")
    u.stepped(2, False)
    assert M.span_slices([u], 8, "euler")[0] == [1] and M.span_slices([u], 8, "euler")[1].tolist() == [1]


# ------------------------------------------------------------------------------------------------------------------ infer layer
def test_option_reaches_sample_units_only_when_a_request_sets_it():
    m = MethodModel()
    plain = [(_clip(200.0), REF_TEXT, "One."), (_clip(300.0), REF_TEXT, "Two.", dict(nfe_step=8))]
    infer.infer_requests(plain, m, Vocoder(), nfe_step=4)
    assert len(m.calls) == 1 and "ode_method" not in m.calls[0]
    n_long = len(infer.request_chunks(REF_TEXT, 2.0, LONG))
    reqs = [(_clip(200.0), REF_TEXT, LONG, dict(ode_method="rk4", nfe_step=8)), (_clip(300.0), REF_TEXT, "Two."),
            (_clip(250.0), REF_TEXT, "Three.", dict(ode_method="euler"))]
    infer.infer_requests(reqs, m, Vocoder(), nfe_step=4)
    assert len(m.calls) == 2 and m.calls[1]["ode_method"] == ["rk4"] * n_long + [None, "euler"] and m.calls[1]["steps"] == [8] * n_long + [4, 4]
    infer.infer_requests([reqs[0]], m, Vocoder(), nfe_step=4)      # all units agree: one name
    assert m.calls[2]["ode_method"] == "rk4"
    with pytest.raises(ValueError, match="unknown request option"):
        infer.infer_requests([(_clip(200.0), REF_TEXT, "One.", dict(ode_methods="rk4"))], m, Vocoder())


def test_models_without_per_unit_grids_get_one_call_per_method():
    class Plain(MethodModel):
        per_unit_time_grids = False

    m = Plain()
    reqs = [(_clip(200.0), REF_TEXT, "One.", dict(ode_method="rk4")), (_clip(300.0), REF_TEXT, "Two."),
            (_clip(250.0), REF_TEXT, "Three.", dict(ode_method="rk4"))]
    infer.infer_requests(reqs, m, Vocoder(), nfe_step=4)
    assert [(c["n"], c.get("ode_method")) for c in m.calls] == [(2, "rk4"), (1, None)] and "ode_method" not in m.calls[1]


def test_process_and_stream_hand_the_method_on():
    m = MethodModel()
    infer.infer_process(_clip(200.0), REF_TEXT, "Short words.", m, Vocoder(), nfe_step=4, show_info=lambda *_: None)
    assert "ode_method" not in m.calls[0]
    infer.infer_process(_clip(200.0), REF_TEXT, "Short words.", m, Vocoder(), nfe_step=4, ode_method="midpoint", show_info=lambda *_: None)
    assert m.calls[1]["ode_method"] == "midpoint"
    m.calls.clear()
    list(infer.infer_process_stream(_clip(200.0), REF_TEXT, LONG, m, Vocoder(), nfe_step=4, ode_method="rk4", show_info=lambda *_: None))
    assert [c["ode_method"] for c in m.calls] == ["rk4", "rk4"]       # the first chunk, then the remaining ones


def test_span_scheduler_plans_every_unit_with_its_method():
    m = MethodModel()
    sched = infer.SpanScheduler(m, Vocoder(), span_steps=2, nfe_step=4)
    n_long = len(infer.request_chunks(REF_TEXT, 2.0, LONG))
    a = sched.admit((_clip(200.0), REF_TEXT, LONG, dict(ode_method="rk4")))
    b = sched.admit((_clip(300.0), REF_TEXT, "Two."))
    c = sched.admit((_clip(300.0), REF_TEXT, "Three.", dict(ode_method="midpoint", nfe_step=2)))
    assert [p.get("ode_method", "absent") for p in m.planned] == ["rk4"] * n_long + ["absent", "midpoint"]
    assert [u.method for u in a.units] == ["rk4"] * n_long and b.units[0].method is None and c.units[0].method == "midpoint"
    done = []
    while sched.busy:
        done += sched.step()
    # span_steps 2 on a Euler handle: 2 steps per span without a method, 1 per span for the RK4 and midpoint units
    assert m.spans[0] == [("rk4", 1)] * n_long + [(None, 2), ("midpoint", 1)]
    assert len(m.spans) == 4 and {id(t) for t in done} == {id(a), id(b), id(c)}


def test_sharded_sampler_hands_every_unit_its_method():
    m = MethodModel()
    sh = serve.ShardedSampler(m)
    reqs = [(_clip(200.0), REF_TEXT, "One.", dict(ode_method="rk4")), (_clip(300.0), REF_TEXT, "Two."),
            (_clip(250.0), REF_TEXT, "Three.", dict(ode_method="euler", cfg_strength=0.5))]
    infer.infer_requests(reqs, sh, Vocoder(), nfe_step=4)
    assert len(m.calls) == 1 and m.calls[0]["ode_method"] == ["rk4", None, "euler"] and m.calls[0]["cfg_strength"] == [2.0, 2.0, 0.5]
    infer.infer_requests([reqs[0]], sh, Vocoder(), nfe_step=4)
    assert m.calls[1]["ode_method"] == "rk4"                         # one name for the job: in the broadcast knobs as it is
    infer.infer_requests([reqs[1]], sh, Vocoder(), nfe_step=4)
    assert "ode_method" not in m.calls[2]
    with pytest.raises(ValueError, match="one name per unit"):
        sh.sample_units(_clip(200.0)[0], [(list("ab"), 120), (list("cd"), 130)], steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, ode_method=["rk4"])


# ------------------------------------------------------------------------------------------------------------------ manager and routes
def _wav(tmp_path, name, freq):
    x = (0.3 * np.sin(2 * np.pi * freq * np.arange(48000) / 24000) * 32767).astype(np.int16)
    p = tmp_path / name
    with wave.open(str(p), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
        f.writeframes(x.tobytes())
    return str(p)


def _edit_body(tmp_path):
    return dict(audio=base64.b64encode(open(_wav(tmp_path, "e.wav", 300), "rb").read()).decode(), text="new words", parts_to_edit=[[0.2, 0.5]])


@pytest.fixture
def app(tmp_path, monkeypatch):
    from fastapi.testclient import TestClient
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", _wav(tmp_path, "a.wav", 200), "reference words")
    model = MethodModel()
    mgr = serve.TTSManager(nfe_step=4, cfg_strength=1.5).load(model, Vocoder())
    seen = []
    real = infer.infer_requests

    def spy(requests, *a, **kw):
        seen.append([r[3] if len(r) > 3 else None for r in requests])
        return real(requests, *a, **kw)

    monkeypatch.setattr(infer, "infer_requests", spy)
    return TestClient(serve.create_app(mgr, reg)), mgr, model, seen, tmp_path


def _routes(tmp_path):
    return [("/v1/audio/speech", dict(text="hello there")), ("/v1/audio/speech/voice", dict(text="hello there", ref_audio_name="KAN_F (Happy)")),
            ("/v1/audio/speech", dict(text="hello there", stream=True)), ("/v1/audio/edit", _edit_body(tmp_path))]


@pytest.mark.parametrize("bad", ["heun", "RK4", ""])
def test_unknown_method_gets_400_on_every_route(app, bad):
    client, mgr, model, seen, tmp_path = app
    for route, body in _routes(tmp_path):
        r = client.post(route, json=dict(body, ode_method=bad))
        assert r.status_code == 400, (route, r.status_code, r.text)
        assert r.json()["detail"] == f"{MSG}{bad!r})", (route, r.json())
    assert model.calls == [] and model.samples == [] and seen == []          # nothing was queued


def test_nfe_step_limit_follows_the_requests_method_on_every_route(app):
    client, mgr, model, seen, tmp_path = app
    for route, body in _routes(tmp_path):
        r = client.post(route, json=dict(body, ode_method="rk4", nfe_step=43))
        assert r.status_code == 400 and "nfe_step must be between 1 and 42 for the rk4 solver (got 43)." in r.json()["detail"], (route, r.text)
    assert model.calls == [] and model.samples == [] and seen == []
    for route, body in _routes(tmp_path):
        assert client.post(route, json=dict(body, ode_method="euler", nfe_step=43)).status_code == 200, route
    model.odeint_kwargs = dict(method="rk4")                # the model's solver bounds a request that names none ...
    assert client.post("/v1/audio/speech", json=dict(text="hi there", nfe_step=43)).status_code == 400
    assert client.post("/v1/audio/speech", json=dict(text="hi there", nfe_step=43, ode_method="euler")).status_code == 200   # ... not one that does


def test_option_reaches_the_model_only_when_the_request_sets_it(app):
    client, mgr, model, seen, tmp_path = app
    assert client.post("/v1/audio/speech", json=dict(text="hello there")).status_code == 200
    assert seen == [[None]] and "ode_method" not in model.calls[0]
    assert client.post("/v1/audio/speech/voice", json=dict(text="hello there", ref_audio_name="KAN_F (Happy)", ode_method="midpoint")).status_code == 200
    assert seen[1] == [dict(ode_method="midpoint")] and model.calls[1]["ode_method"] == "midpoint"
    # the edit route: `sample()` gets the keyword only when the request names a solver
    assert client.post("/v1/audio/edit", json=_edit_body(tmp_path)).status_code == 200
    assert "ode_method" not in model.samples[0]
    assert client.post("/v1/audio/edit", json=dict(_edit_body(tmp_path), ode_method="rk4", nfe_step=6)).status_code == 200
    assert model.samples[1]["ode_method"] == "rk4" and model.samples[1]["steps"] == 6
    # the manager's keywords
    mgr.synthesize("hello there", ref_audio_path=_wav(tmp_path, "a.wav", 200), ref_text="reference words", ode_method="rk4", nfe_step=2)
    assert seen[-1] == [dict(nfe_step=2, ode_method="rk4")] and model.calls[-1]["ode_method"] == "rk4"
    with pytest.raises(ValueError, match="ode_method must be one of"):
        mgr.edit(_clip(200.0), "new words", [[0.2, 0.5]], ode_method="heun")


def test_streamed_tail_keeps_the_heads_method(app):
    client, mgr, model, seen, tmp_path = app
    pieces = list(mgr.synthesize_stream(LONG, ref_audio_path=_wav(tmp_path, "a.wav", 200), ref_text="reference words", ode_method="rk4", nfe_step=3))
    assert len(pieces) >= 2
    assert seen == [[dict(nfe_step=3, ode_method="rk4")]] * 2                  # head, then tail: the same options
    assert [c["ode_method"] for c in model.calls] == ["rk4", "rk4"] and model.calls[1]["n"] >= 1
    r = client.post("/v1/audio/speech", json=dict(text=LONG, stream=True, ode_method="midpoint"))
    assert r.status_code == 200 and [c["ode_method"] for c in model.calls[2:]] == ["midpoint", "midpoint"]
