"""CPU: the C-ABI library loads and exports every symbol include/f5hip.h declares (no compute without a GPU);
the multi-GPU layer (unit sharding, broadcast of reference latents, waveform gather) on gloo, world_size 2."""
import ctypes
import os
import re
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from tts_indic_server_f5_amd import _lib, build
    path = build.build(verbose=False)
    lib = ctypes.CDLL(path)
    header = open(os.path.join(ROOT, "include", "f5hip.h")).read()
    declared = set(re.findall(r"\b(f5hip_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in declared:
        getattr(lib, name)
    lib.f5hip_abi_version.restype = ctypes.c_int
    assert lib.f5hip_abi_version() == 1


def test_no_cpu_fallback_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tts_indic_server_f5_amd import _lib, synth
    from tts_indic_server_f5_amd.model import DiTArch, F5HipModel
    arch = dict(dim=128, depth=1, heads=2, ff_mult=2, text_dim=64, conv_layers=1, text_num_embeds=8)
    with pytest.raises((_lib.F5HipError, RuntimeError, AssertionError)):
        F5HipModel(DiTArch(**arch), synth.dit_state_dict(**arch), device="cuda:0")
    with pytest.raises(_lib.F5HipError):
        F5HipModel(DiTArch(**arch), synth.dit_state_dict(**arch), device="cpu")


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "tts-indic-server-f5_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip")):
                src = open(os.path.join(dirpath, f), encoding="utf-8").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f


def test_shard_units_balanced_and_deterministic():
    from tts_indic_server_f5_amd.sharding import shard_units, unit_cost
    frames = [1404] * 64
    sh = shard_units(frames, 8)
    assert sorted(sum(sh, [])) == list(range(64)) and all(len(s) == 8 for s in sh)
    ragged = [700 + 37 * ((i * 7919) % 40) for i in range(61)]
    sh = shard_units(ragged, 8)
    assert sorted(sum(sh, [])) == list(range(61))
    loads = [sum(unit_cost(ragged[i]) for i in s) for s in sh]
    assert max(loads) / (sum(loads) / 8) < 1.08
    assert sh == shard_units(ragged, 8)


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from tts_indic_server_f5_amd.sharding import broadcast_ref_latents, gather_waves, shard_units
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(469, 100, generator=g) if rank == 0 else None
    ids = torch.randint(0, 2545, (60,), generator=g) if rank == 0 else None
    c, i = broadcast_ref_latents(cond, ids, torch.device("cpu"))
    ok = c.shape == (469, 100) and i.shape == (60,) and i.dtype == torch.int64
    g2 = torch.Generator().manual_seed(3)
    ok = ok and torch.equal(c, torch.randn(469, 100, generator=g2)) and torch.equal(i, torch.randint(0, 2545, (60,), generator=g2))
    mine = shard_units([1404, 900, 1200, 700, 1404], world)[rank]
    wave = torch.full((1000 + 100 * rank,), float(rank))
    got = gather_waves(wave, dst=0)
    if rank == 0:
        ok = ok and len(got) == world and all(got[r].numel() == 1000 + 100 * r and float(got[r][5]) == r for r in range(world))
    else:
        ok = ok and got is None
    q.put((rank, bool(ok), mine))
    dist.barrier()
    dist.destroy_process_group()


def test_broadcast_and_gather_gloo_world2():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _ in res), res
    assert sorted(res[0][2] + res[1][2]) == [0, 1, 2, 3, 4]


def test_bench_launcher_spawns_one_rank_per_gpu():
    """`python bench.py --gpus 2` (no torchrun environment) must start 2 fresh ranks itself, form the process group and report
    n_gpus from its world size; F5HIP_BENCH_FAKE=1 skips the GPU work so this runs on CPU (gloo)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["F5HIP_BENCH_FAKE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--mode", "strong"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["value"] == 3.0 and d["steps"] == 3 and d["mode"] == "strong"   # sum over ranks of (rank + 1)


def test_bench_under_torch_distributed_run():
    """The driver's own N > 1 invocation: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P
    bench.py --gpus N ...` -- bench.py must join the group torchrun made (no second spawn) and rank 0 alone prints the JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["F5HIP_BENCH_FAKE"] = "1"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                            # one line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] == 3.0 and d["steps"] == 3


def test_bench_launcher_does_not_hang_when_a_rank_dies():
    """a rank that exits before its first collective leaves the others blocked in it; the launcher polls every child, gives the
    survivors a grace period, terminates them and returns non-zero, with the dead rank's stderr kept (gpurun_out/bench_rank<r>.err)."""
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["F5HIP_BENCH_FAKE"] = "1"
    env["F5HIP_BENCH_FAKE_FAIL_RANK"] = "1"
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env, capture_output=True,
                       text=True, timeout=180)
    assert r.returncode != 0 and time.time() - t0 < 120
    assert "rank 1 exit code 3" in r.stderr and "fake failure of rank 1" in r.stderr


def test_bench_dump_outputs_is_exact_or_a_fixed_sample_under_64_mb(tmp_path):
    """--dump-outputs: one float32 wave_<k>.npy per returned waveform; exact when they fit, otherwise the same seeded sample positions on every
    run (so two builds compare sample for sample) and under 64 MB in all.  --steps below 1 is rejected, not run as an empty timed region."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    assert bench.parse_args(["--steps", "7", "--dump-outputs", str(tmp_path)]).steps == 7
    g = torch.Generator().manual_seed(0)
    small = [torch.randn(1000, generator=g), torch.randn(1700, generator=g)]
    bench.dump_outputs(small, str(tmp_path / "small"))
    for k, w in enumerate(small):
        got = np.load(tmp_path / "small" / f"wave_{k:03d}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, w.numpy())
    big = [torch.randn(n, generator=g) for n in (9_000_000, 8_000_000)]      # 68 MB of float32
    for d in ("a", "b"):
        bench.dump_outputs(big, str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["wave_000.npy", "wave_001.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64e6
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    assert np.isin(np.load(tmp_path / "a" / "wave_001.npy"), big[1].numpy()).all()


def test_strong_mode_sharding_covers_every_unit_once():
    from tts_indic_server_f5_amd.sharding import shard_units, unit_cost
    frames = [1404] * 64
    for world in (1, 2, 4, 8):
        sh = shard_units(frames, world)
        assert sorted(sum(sh, [])) == list(range(64)) and {len(s) for s in sh} == {64 // world}
    import random
    rnd = random.Random(3)
    ragged = [468 + rnd.randint(562, 1312) for _ in range(64)]          # U(6 s, 14 s) generated frames
    sh = shard_units(ragged, 8)
    loads = [sum(unit_cost(ragged[i]) for i in s) for s in sh]
    assert sorted(sum(sh, [])) == list(range(64)) and max(loads) / min(loads) < 1.08   # LPT dealing balances the cost model


def test_torch_library_ops_register_without_a_gpu():
    """north_star: "host Python calling HIP through PyTorch-ROCm custom ops".  csrc/torch_ops.cpp registers the hot path with TORCH_LIBRARY over
    the C ABI; the extension must load here (no GPU) and expose the documented schemas (no compute calls: that is tests/test_gpu_dit.py)."""
    import torch
    from tts_indic_server_f5_amd import torch_ops
    assert torch_ops.load(), f"{torch_ops.TORCH_LIB_PATH} missing: run __graft_entry__.build()"
    schemas = {name: str(getattr(torch.ops.f5hip, name).default._schema) for name in ("cfm_sample", "vocos_decode", "bigvgan_forward")}
    assert schemas["cfm_sample"] == ("f5hip::cfm_sample(int handle, Tensor dur, Tensor? kv_len, Tensor cond, Tensor cond_mask, Tensor text, Tensor y0, "
                                     "Tensor t_grid, float cfg_strength) -> Tensor")
    assert schemas["vocos_decode"] == "f5hip::vocos_decode(int handle, Tensor mel, int hop_length) -> Tensor"
    assert schemas["bigvgan_forward"] == "f5hip::bigvgan_forward(int handle, Tensor mel, int total_upsample) -> Tensor"
    with pytest.raises(RuntimeError, match="must be a contiguous fp32 tensor on the HIP device"):   # argument checks run before any device work
        torch.ops.f5hip.vocos_decode(0, torch.zeros(1, 100, 8), 256)


# the schemas of the wave operators as the TORCH_LIBRARY block registers them: part of the interface
WAVE_OP_SCHEMAS = {
    "wave_encode": "f5hip::wave_encode(Tensor[] pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, int new_freq, int encoding, Tensor? taps) -> "
                   "(Tensor, Tensor, Tensor)",
    "wave_flac": "f5hip::wave_flac(Tensor[] pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, int sample_rate) -> (Tensor, Tensor, Tensor)",
    "wave_flac_levels": "f5hip::wave_flac_levels(Tensor[] pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, int sample_rate, Tensor level) -> "
                        "(Tensor, Tensor, Tensor)",
    "wave_loudness": "f5hip::wave_loudness(Tensor(a!) pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, Tensor gain_k) -> Tensor",
    "wave_prosody": "f5hip::wave_prosody(Tensor pcm, Tensor in_off, Tensor max_len, Tensor? len_dev, Tensor stretch_p, Tensor stretch_q, Tensor pitch, "
                    "Tensor? taps) -> (Tensor, Tensor, Tensor, Tensor)",
}


def test_wave_operators_report_their_own_name_from_the_shared_checks():
    """The wave operators check their request table (pcm, in_off, max_len, len_dev) in one shared helper of csrc/torch_ops.cpp: a refusal must
    still name the operator that was called, not the helper, and must come before any device call (there is no device here).  Two requests,
    `in_off` one element short, then a host tensor as `pcm`.  wave_flac_levels shares wave_flac's body and reports the table as wave_flac."""
    import torch
    from tts_indic_server_f5_amd import torch_ops
    assert torch_ops.load(), f"{torch_ops.TORCH_LIB_PATH} missing: run __graft_entry__.build()"
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)   # noqa: E731
    pcm, io, ml = torch.zeros(64, dtype=torch.int16), torch.zeros(2, dtype=torch.int64), i32(16, 16)
    calls = {
        "wave_encode": lambda p, o: torch.ops.f5hip.wave_encode([p], o, ml, None, 24000, 0, None),
        "wave_flac": lambda p, o: torch.ops.f5hip.wave_flac([p], o, ml, None, 24000),
        "wave_flac_levels": lambda p, o: torch.ops.f5hip.wave_flac_levels([p], o, ml, None, 24000, i32(0, 1)),
        "wave_loudness": lambda p, o: torch.ops.f5hip.wave_loudness(p, o, ml, None, torch.zeros(2, dtype=torch.float64)),
        "wave_prosody": lambda p, o: torch.ops.f5hip.wave_prosody(p, o, ml, None, i32(1, 1), i32(1, 1), i32(0, 0), None),
    }
    assert set(calls) == set(WAVE_OP_SCHEMAS)
    for name, call in calls.items():
        assert str(getattr(torch.ops.f5hip, name).default._schema) == WAVE_OP_SCHEMAS[name]
        said = "wave_flac" if name == "wave_flac_levels" else name
        for args, words in (((pcm, io[:1]), "one value per request"), ((pcm, io), "HIP device")):
            with pytest.raises(RuntimeError) as e:
                call(*args)
            assert f"f5hip::{said}: " in str(e.value) and words in str(e.value), (name, words, str(e.value))
