"""CPU: per-request sampler settings (`speed`, `nfe_step`, `cfg_strength`, `sway_sampling_coef`, `seed`) on stand-in samplers -- the
400s of the three routes, the defaults of omitted fields, grouping by time grid in `infer.infer_requests`, per-unit CFG strengths in unit
order, seeded noise that does not depend on the batch, and the per-unit knobs of a gloo world-2 `serve.ShardedSampler` job."""
import base64
import os
import socket
import sys
import wave

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tts_indic_server_f5_amd import infer, serve  # noqa: E402
from tts_indic_server_f5_amd.model import unit_duration  # noqa: E402


class KnobModel:
    """`sample_units` of F5HipModel in closed form: records every call's knobs; a unit's mel is its noise when it has a noise source (a
    generator: drawn at the unit's final duration like F5HipModel does; or `y0`), else a ramp."""
    device = torch.device("cpu")
    odeint_kwargs = dict(method="euler")

    def __init__(self):
        self.calls = []

    def cond_mel(self, audio):
        n = audio.shape[-1] // 256 + 1
        return audio[0, : (n - 1) * 256].reshape(n - 1, 256).mean(1, keepdim=True).repeat(1, 100)[None]

    def sample_units(self, audio, units, *, steps, cfg_strength, sway_sampling_coef, seed=None, generators=None, y0=None):
        audios = list(audio) if isinstance(audio, (list, tuple)) else [audio] * len(units)
        self.calls.append(dict(n=len(units), frames=[f for _, f in units], keys=["".join(t) + f"|{f}" for t, f in units], steps=steps, cfg=cfg_strength, sway=sway_sampling_coef,
                               generators=generators, y0=y0))
        out = []
        for i, (a, (tokens, frames)) in enumerate(zip(audios, units)):
            mel = self.cond_mel(a) if a.ndim == 2 else a
            dur = unit_duration(mel.shape[1], len(tokens), frames)
            if y0 is not None and y0[i] is not None:
                out.append(y0[i][:dur].clone())
            elif generators is not None and generators[i] is not None:
                out.append(torch.randn(dur, 100, generator=generators[i]))
            else:
                out.append(torch.linspace(-1, 1, dur * 100).reshape(dur, 100) * (steps + 1))
        self.calls[-1]["noise"] = [o.clone() for o in out]
        return out


class Vocoder:
    def __init__(self):
        self.ragged_calls = []

    def decode(self, mel):
        t = mel.shape[-1]
        return (torch.sin(torch.arange(256 * (t - 1), dtype=torch.float32) * 0.01) * mel.mean() * 3)[None]

    def decode_ragged(self, mels):
        self.ragged_calls.append(len(mels))
        return [self.decode(m[None])[0] for m in mels]


def _clip(freq, seconds=2.0, amp=0.3):
    return (amp * torch.sin(2 * torch.pi * freq * torch.arange(int(24000 * seconds)) / 24000))[None], 24000


REF_TEXT = "Hi there."
LONG = ("The quick brown fox jumps over the lazy dog. Pack my box with five dozen liquor jugs. How vexingly quick daft zebras jump. "
        "Sphinx of black quartz, judge my vow. The five boxing wizards jump quickly. Jackdaws love my big sphinx of quartz.")


# ------------------------------------------------------------------------------------------------------------------ infer layer
def test_speed_changes_planned_frames():
    m = KnobModel()
    infer.infer_requests([(_clip(200.0), REF_TEXT, "Short words here.", dict(speed=0.5)),
                          (_clip(200.0), REF_TEXT, "Short words here.")], m, Vocoder(), nfe_step=4)
    ref_frames = 24000 * 2 // 256
    slow, normal = m.calls[0]["frames"]
    assert m.calls[0]["n"] == 2 and abs((slow - ref_frames) - 2 * (normal - ref_frames)) <= 2


def test_two_time_grids_make_two_sampler_calls_and_one_ragged_vocode():
    m, v = KnobModel(), Vocoder()
    reqs = [(_clip(200.0), REF_TEXT, LONG, dict(nfe_step=8)), (_clip(300.0), REF_TEXT, "Two."), (_clip(250.0), REF_TEXT, "Three.", dict(nfe_step=8))]
    out = infer.infer_requests(reqs, m, v, nfe_step=4)
    n_long = len(infer.request_chunks(REF_TEXT, 2.0, LONG))
    assert [(c["steps"], c["n"]) for c in m.calls] == [(8, n_long + 1), (4, 1)]
    assert v.ragged_calls == [n_long + 2] and len(out) == 3
    # a request's result is what it gets alone
    for r, (w, _, _) in zip(reqs, out):
        alone = infer.infer_requests([r], KnobModel(), Vocoder(), nfe_step=4)[0][0]
        np.testing.assert_array_equal(w, alone)


def test_per_unit_cfg_reaches_sample_units_in_unit_order():
    m = KnobModel()
    reqs = [(_clip(200.0), REF_TEXT, LONG, dict(cfg_strength=3.5)), (_clip(300.0), REF_TEXT, "Two.", dict(cfg_strength=0.0)),
            (_clip(250.0), REF_TEXT, "Three.")]
    infer.infer_requests(reqs, m, Vocoder(), nfe_step=4, cfg_strength=2.0)
    n_long = len(infer.request_chunks(REF_TEXT, 2.0, LONG))
    assert len(m.calls) == 1 and m.calls[0]["cfg"] == [3.5] * n_long + [0.0, 2.0]
    m2 = KnobModel()   # all equal: one float, today's call
    infer.infer_requests(reqs[2:], m2, Vocoder(), nfe_step=4, cfg_strength=2.0)
    assert m2.calls[0]["cfg"] == 2.0 and m2.calls[0]["generators"] is None


def test_seed_noise_is_independent_of_the_batch_and_leaves_the_global_generator():
    torch.manual_seed(123)
    state = torch.get_rng_state()
    seeded = (_clip(200.0), REF_TEXT, LONG, dict(seed=42))
    m1, m2 = KnobModel(), KnobModel()
    alone = infer.infer_requests([seeded], m1, Vocoder(), nfe_step=4)[0][0]
    assert torch.equal(torch.get_rng_state(), state)                # only unseeded units touch the global generator
    batched = infer.infer_requests([(_clip(300.0), REF_TEXT, "Other words.", dict(seed=7)), (_clip(300.0), REF_TEXT, "Unseeded."), seeded],
                                   m2, Vocoder(), nfe_step=4)[2][0]
    np.testing.assert_array_equal(alone, batched)
    n0 = m1.calls[0]["noise"]
    assert len(n0) >= 3 and not torch.equal(n0[0][:50], n0[1][:50])   # chunk 1's noise differs from chunk 0's
    g = torch.Generator().manual_seed(42)
    assert torch.equal(n0[0], torch.randn(n0[0].shape[0], 100, generator=g))
    assert torch.equal(n0[1], torch.randn(n0[1].shape[0], 100, generator=g))   # chunk 1: after chunk 0's draws
    assert torch.equal(m2.calls[0]["noise"][2], n0[0])


def test_stream_with_seed_equals_unstreamed_with_seed():
    a = _clip(200.0)
    w, _, _ = infer.infer_process(a, REF_TEXT, LONG, KnobModel(), Vocoder(), nfe_step=4, seed=9, show_info=lambda *_: None)
    pieces = list(infer.infer_process_stream(a, REF_TEXT, LONG, KnobModel(), Vocoder(), nfe_step=4, seed=9, show_info=lambda *_: None))
    np.testing.assert_array_equal(np.concatenate(pieces), w.astype(np.float32))


def test_continued_generator_moves_only_on_success():
    g = torch.Generator().manual_seed(5)
    state = g.get_state()

    class Failing(KnobModel):
        def sample_units(self, *a, **k):
            super().sample_units(*a, **k)
            raise RuntimeError("device gone")

    with pytest.raises(RuntimeError):
        infer.infer_requests([(_clip(200.0), REF_TEXT, ["Chunk."], dict(generator=g))], Failing(), Vocoder())
    assert torch.equal(g.get_state(), state)
    infer.infer_requests([(_clip(200.0), REF_TEXT, ["Chunk."], dict(generator=g))], KnobModel(), Vocoder())
    assert not torch.equal(g.get_state(), state)


# ------------------------------------------------------------------------------------------------------------------ routes
def _wav(tmp_path, name, freq):
    x = (0.3 * np.sin(2 * np.pi * freq * np.arange(48000) / 24000) * 32767).astype(np.int16)
    p = tmp_path / name
    with wave.open(str(p), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(24000)
        f.writeframes(x.tobytes())
    return str(p)


@pytest.fixture
def app(tmp_path, monkeypatch):
    from fastapi.testclient import TestClient
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", _wav(tmp_path, "a.wav", 200), "reference words")
    model = KnobModel()
    mgr = serve.TTSManager(nfe_step=4, cfg_strength=1.5).load(model, Vocoder())
    seen = []
    real = infer.infer_requests

    def spy(requests, *a, **kw):
        seen.append(([r[3] if len(r) > 3 else None for r in requests], kw))
        return real(requests, *a, **kw)

    monkeypatch.setattr(infer, "infer_requests", spy)
    edits = []
    monkeypatch.setattr(mgr, "edit", lambda *a, **kw: edits.append(kw) or np.zeros(2400, dtype=np.float32))
    return TestClient(serve.create_app(mgr, reg)), mgr, model, seen, edits, tmp_path


def _edit_body(tmp_path):
    return dict(audio=base64.b64encode(open(_wav(tmp_path, "e.wav", 300), "rb").read()).decode(), text="new words", parts_to_edit=[[0.2, 0.5]])


BAD = [("speed", 0, "speed must be greater than 0"), ("speed", -1.5, "speed must be greater than 0"),
       ("speed", "Infinity", "speed must be a finite number"), ("speed", "NaN", "speed must be a finite number"),
       ("nfe_step", 0, "nfe_step must be between 1 and 128 for the euler solver"),
       ("nfe_step", 129, "nfe_step must be between 1 and 128 for the euler solver"),
       ("cfg_strength", "NaN", "cfg_strength must be a finite number"),
       ("sway_sampling_coef", "-Infinity", "sway_sampling_coef must be a finite number"),
       ("seed", -1, "seed must be between 0 and 2**63 - 1"), ("seed", 2 ** 63, "seed must be between 0 and 2**63 - 1")]


def _post(client, route, body, field, value):
    import json
    raw = json.dumps(dict(body, **{field: 0})).replace(f'"{field}": 0', f'"{field}": {value}')   # NaN / Infinity as JSON literals
    return client.post(route, content=raw, headers={"content-type": "application/json"})


@pytest.mark.parametrize("field,value,msg", BAD)
def test_invalid_fields_get_400_on_every_route(app, field, value, msg):
    client, mgr, model, seen, edits, tmp_path = app
    routes = [("/v1/audio/speech", dict(text="hello there")), ("/v1/audio/speech/voice", dict(text="hello there", ref_audio_name="KAN_F (Happy)")),
              ("/v1/audio/speech", dict(text="hello there", stream=True))]
    if field != "speed":
        routes.append(("/v1/audio/edit", _edit_body(tmp_path)))
    for route, body in routes:
        r = _post(client, route, body, field, value)
        assert r.status_code == 400, (route, r.status_code, r.text)
        assert msg in r.json()["detail"], (route, r.json())
    assert model.calls == [] and seen == [] and edits == []          # nothing was queued


def test_nfe_step_limit_follows_the_ode_method(app):
    client, mgr, model, seen, edits, tmp_path = app
    for method, hi in (("midpoint", 64), ("rk4", 42)):
        model.odeint_kwargs = dict(method=method)
        assert _post(client, "/v1/audio/speech", dict(text="hi there"), "nfe_step", hi + 1).status_code == 400
        assert f"between 1 and {hi} for the {method} solver" in _post(client, "/v1/audio/speech", dict(text="hi"), "nfe_step", hi + 1).json()["detail"]
        assert _post(client, "/v1/audio/speech", dict(text="hi there"), "nfe_step", hi).status_code == 200


def test_edit_route_has_no_speed(app):
    client, mgr, model, seen, edits, tmp_path = app
    r = client.post("/v1/audio/edit", json=dict(_edit_body(tmp_path), nfe_step=6, cfg_strength=0.5, seed=3))
    assert r.status_code == 200 and edits == [dict(nfe_step=6, cfg_strength=0.5, seed=3)]


def test_speed_half_reaches_the_sampler_with_twice_the_generated_frames(app):
    client, mgr, model, seen, edits, tmp_path = app
    for route, body in [("/v1/audio/speech", dict(text="hello there friend")),
                        ("/v1/audio/speech/voice", dict(text="hello there friend", ref_audio_name="KAN_F (Happy)"))]:
        model.calls.clear()
        assert client.post(route, json=dict(body, speed=1)).status_code == 200
        assert client.post(route, json=dict(body, speed=0.5)).status_code == 200
        ref_frames = next(iter(mgr._prep_cache.values()))[0].ref_frames   # the prepared (trimmed) prompt's frames
        gen1, gen2 = (c["frames"][0] - ref_frames for c in model.calls)
        assert abs(gen2 - 2 * gen1) <= 2 and gen1 > 10


def test_omitted_fields_reach_infer_requests_as_the_manager_defaults(app):
    client, mgr, model, seen, edits, tmp_path = app
    assert client.post("/v1/audio/speech", json=dict(text="hello there")).status_code == 200
    (opts, kw), = seen
    assert opts == [None] and {k: kw[k] for k in mgr.opts} == mgr.opts == dict(nfe_step=4, cfg_strength=1.5, sway_sampling_coef=-1.0, speed=1.0)
    assert model.calls[0]["steps"] == 4 and model.calls[0]["cfg"] == 1.5 and model.calls[0]["generators"] is None
    assert client.post("/v1/audio/speech", json=dict(text="hello there", nfe_step=7, seed=5)).status_code == 200
    assert seen[1][0] == [dict(nfe_step=7, seed=5)]


def test_same_seed_same_response(app):
    client, mgr, model, seen, edits, tmp_path = app
    a = client.post("/v1/audio/speech", json=dict(text="hello there", seed=77)).content
    b = client.post("/v1/audio/speech", json=dict(text="hello there", seed=77)).content
    c = client.post("/v1/audio/speech", json=dict(text="hello there", seed=78)).content
    assert a == b and a != c


# ------------------------------------------------------------------------------------------------------------------ world size 2
def _by_value(tensors):
    """numpy copies for the result queue: a torch tensor put on a torch.multiprocessing queue is shared through the SENDER's resource
    sharer, which is gone once the rank process has exited, so the parent could not unpickle it."""
    return [t.numpy().copy() for t in tensors]


def _rank(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from tts_indic_server_f5_amd import infer as I, serve as S
    local = KnobModel()
    if rank != 0:
        S.rank_worker_loop(local)
        q.put((rank, [(c["keys"], c["cfg"], _by_value(c["noise"])) for c in local.calls]))
    else:
        sh = S.ShardedSampler(local)
        reqs = [(_clip(200.0), REF_TEXT, LONG, dict(cfg_strength=3.0, seed=4)), (_clip(330.0, 4.0), "second voice says", "Some words.",
                                                                                 dict(cfg_strength=0.0)),
                (_clip(250.0), REF_TEXT, "Third one here.", dict(seed=8))]
        got = I.infer_requests(reqs, sh, Vocoder(), nfe_step=4, cfg_strength=2.0)
        ref_model = KnobModel()
        ref = I.infer_requests(reqs, ref_model, Vocoder(), nfe_step=4, cfg_strength=2.0)
        seeded_ok = all(np.array_equal(got[i][0], ref[i][0]) for i in (0, 2))
        sh.close()
        c = ref_model.calls[0]
        q.put((rank, dict(seeded_ok=seeded_ok, cfg=c["cfg"], keys=c["keys"], noise=_by_value(c["noise"]),
                          mine=[(cc["keys"], cc["cfg"], _by_value(cc["noise"])) for cc in local.calls])))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_world2_delivers_per_unit_knobs_and_seeded_noise():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    r0 = res[0]
    assert r0["seeded_ok"]
    n_long = len(infer.request_chunks(REF_TEXT, 2.0, LONG))
    seeded = set(range(n_long)) | {n_long + 1}
    # every unit reached exactly one rank with its own cfg strength and -- when seeded -- the noise the single process drew for it
    assert len(set(r0["keys"])) == len(r0["keys"])
    seen = set()
    for calls in (r0["mine"], res[1]):
        assert len(calls) == 1
        keys, cfg, noise = calls[0]
        assert isinstance(cfg, list) and len(cfg) == len(keys)
        for key, c, nz in zip(keys, cfg, noise):
            i = r0["keys"].index(key)
            seen.add(i)
            assert c == r0["cfg"][i]
            if i in seeded:
                assert np.array_equal(nz, r0["noise"][i])
    assert len(seen) == len(r0["keys"]) and len(res[1][0][0]) > 0 and len(r0["mine"][0][0]) > 0
