"""CPU: one sampler call for units of different time grids.  A model that declares `per_unit_time_grids` gets ONE `sample_units` call from
`infer.infer_requests` with per-unit `steps` / `sway_sampling_coef` lists in unit order (and one ragged vocode); a gloo world-2
`serve.ShardedSampler` hands every rank its own units' grids and returns the mels in request order; the routes take mixed `nfe_step`
values from concurrent requests."""
import os
import socket
import sys
import threading

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tts_indic_server_f5_amd import infer, serve  # noqa: E402
from tts_indic_server_f5_amd.model import F5HipModel, per_unit_values  # noqa: E402
from test_request_knobs import LONG, REF_TEXT, KnobModel, Vocoder, _clip, _wav  # noqa: E402


class GridModel(KnobModel):
    """KnobModel that samples units of different time grids in one call, as F5HipModel does: a unit's mel without a noise source is a
    ramp scaled by its own step count and sway."""
    per_unit_time_grids = True

    def sample_units(self, audio, units, *, steps, cfg_strength, sway_sampling_coef, seed=None, generators=None, y0=None):
        n = len(units)
        steps_u = steps if isinstance(steps, list) else [steps] * n
        sway_u = sway_sampling_coef if isinstance(sway_sampling_coef, list) else [sway_sampling_coef] * n
        out = super().sample_units(audio, units, steps=0, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed,
                                   generators=generators, y0=y0)
        self.calls[-1]["steps"] = steps
        for i in range(n):
            if (y0 is None or y0[i] is None) and (generators is None or generators[i] is None):
                out[i] = out[i] * (steps_u[i] + 1) + (0.0 if sway_u[i] is None else sway_u[i])
        self.calls[-1]["noise"] = [o.clone() for o in out]
        return out


def test_f5hip_model_declares_per_unit_time_grids():
    assert F5HipModel.per_unit_time_grids is True
    assert per_unit_values(8, 3, "steps") == 8 and per_unit_values([8, 4, 8], 3, "steps") == [8, 4, 8]
    assert per_unit_values(torch.tensor([1.0, -1.0]), 2, "sway") == [1.0, -1.0]
    with pytest.raises(ValueError, match="one value per unit"):
        per_unit_values([8, 4], 3, "steps")


def test_per_unit_grids_make_one_sampler_call_and_one_ragged_vocode():
    m, v = GridModel(), Vocoder()
    reqs = [(_clip(200.0), REF_TEXT, LONG, dict(nfe_step=8)), (_clip(300.0), REF_TEXT, "Two.", dict(sway_sampling_coef=None)),
            (_clip(250.0), REF_TEXT, "Three.", dict(nfe_step=16, sway_sampling_coef=0.5))]
    out = infer.infer_requests(reqs, m, v, nfe_step=4, sway_sampling_coef=-1.0)
    n_long = len(infer.request_chunks(REF_TEXT, 2.0, LONG))
    assert len(m.calls) == 1 and m.calls[0]["n"] == n_long + 2
    assert m.calls[0]["steps"] == [8] * n_long + [4, 16]
    assert m.calls[0]["sway"] == [-1.0] * n_long + [None, 0.5]
    assert v.ragged_calls == [n_long + 2] and len(out) == 3
    for r, (w, _, _) in zip(reqs, out):   # a request's result is what it gets alone
        alone = infer.infer_requests([r], GridModel(), Vocoder(), nfe_step=4, sway_sampling_coef=-1.0)[0][0]
        np.testing.assert_array_equal(w, alone)
    # one grid for all: the knobs stay scalars, as before
    m1 = GridModel()
    infer.infer_requests(reqs[:2], m1, Vocoder(), nfe_step=8, sway_sampling_coef=None)
    assert len(m1.calls) == 1 and m1.calls[0]["steps"] == 8 and m1.calls[0]["sway"] is None


def test_unseeded_units_draw_noise_in_flat_request_order():
    """With one call for every grid, unseeded units draw from the global generator unit by unit in request order."""
    class Drawing(GridModel):
        def sample_units(self, audio, units, **kw):
            self.draws = [torch.randn(1).item() for _ in units]
            return super().sample_units(audio, units, **kw)

    reqs = [(_clip(200.0), REF_TEXT, "First request.", dict(nfe_step=16)), (_clip(300.0), REF_TEXT, "Second one.", dict(nfe_step=4)),
            (_clip(250.0), REF_TEXT, "Third.", dict(nfe_step=16))]
    m = Drawing()
    torch.manual_seed(3)
    infer.infer_requests(reqs, m, Vocoder(), nfe_step=4)
    torch.manual_seed(3)
    expect = [torch.randn(1).item() for _ in range(3)]
    assert len(m.calls) == 1 and m.draws == expect and m.calls[0]["steps"] == [16, 4, 16]


# ------------------------------------------------------------------------------------------------------------------ routes
def test_routes_accept_mixed_nfe_step_from_concurrent_requests(tmp_path):
    from fastapi.testclient import TestClient
    reg = serve.VoiceRegistry()
    reg.add("KAN_F (Happy)", _wav(tmp_path, "a.wav", 200), "reference words")
    model = GridModel()
    mgr = serve.TTSManager(nfe_step=4, micro_batch=dict(max_requests=8, max_wait_ms=300)).load(model, Vocoder())
    try:
        client = TestClient(serve.create_app(mgr, reg))
        bodies = [("/v1/audio/speech", dict(text="hello there", nfe_step=5)),
                  ("/v1/audio/speech/voice", dict(text="hello there friend", ref_audio_name="KAN_F (Happy)", nfe_step=9)),
                  ("/v1/audio/speech", dict(text="and one more", nfe_step=16, sway_sampling_coef=0.0))]
        codes, barrier = [None] * 3, threading.Barrier(3)

        def post(i):
            barrier.wait()
            codes[i] = client.post(bodies[i][0], json=bodies[i][1]).status_code

        threads = [threading.Thread(target=post, args=(i,)) for i in range(3)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert codes == [200, 200, 200]
        seen = set()
        for c in model.calls:
            seen |= set(c["steps"]) if isinstance(c["steps"], list) else {c["steps"]}
        assert {5, 9, 16} <= seen
    finally:
        mgr.close()


# ------------------------------------------------------------------------------------------------------------------ world size 2
def _rank(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from tts_indic_server_f5_amd import infer as I, serve as S
    local = GridModel()
    if rank != 0:
        S.rank_worker_loop(local)
        q.put((rank, [(c["keys"], c["steps"], c["sway"]) for c in local.calls]))
    else:
        sh = S.ShardedSampler(local)
        reqs = [(_clip(200.0), REF_TEXT, LONG, dict(nfe_step=8, seed=4)), (_clip(330.0, 4.0), "second voice says", "Some words.",
                                                                           dict(nfe_step=16, sway_sampling_coef=None)),
                (_clip(250.0), REF_TEXT, "Third one here.", dict(sway_sampling_coef=0.5, seed=8))]
        got = I.infer_requests(reqs, sh, Vocoder(), nfe_step=4)
        ref_model = GridModel()
        ref = I.infer_requests(reqs, ref_model, Vocoder(), nfe_step=4)
        same = all(np.array_equal(got[i][0], ref[i][0]) for i in range(3))
        sh.close()
        c = ref_model.calls[0]
        q.put((rank, dict(flag=sh.per_unit_time_grids, same=same, n_calls=len(ref_model.calls), keys=c["keys"], steps=c["steps"],
                          sway=c["sway"], mine=[(cc["keys"], cc["steps"], cc["sway"]) for cc in local.calls])))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_world2_slices_per_unit_grids_and_keeps_request_order():
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
    assert r0["flag"] is True and r0["n_calls"] == 1 and r0["same"]   # gathered mels in request order, as one process computes them
    n_long = len(infer.request_chunks(REF_TEXT, 2.0, LONG))
    assert r0["steps"] == [8] * n_long + [16, 4] and r0["sway"] == [-1.0] * n_long + [None, 0.5]
    seen = set()
    for calls in (r0["mine"], res[1]):
        assert len(calls) == 1
        keys, steps, sway = calls[0]
        assert isinstance(steps, list) and len(steps) == len(keys) and isinstance(sway, list) and len(sway) == len(keys)
        for key, st, sw in zip(keys, steps, sway):
            i = r0["keys"].index(key)
            seen.add(i)
            assert st == r0["steps"][i] and sw == r0["sway"][i]
    assert len(seen) == len(r0["keys"])
