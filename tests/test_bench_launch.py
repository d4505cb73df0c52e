"""bench.py's launch path without a GPU (VERDICT r3 missing #2): `python bench.py --gpus 2` started PLAINLY must spawn its own
ranks (torch.distributed.run, 127.0.0.1), and exactly one JSON line must come back from rank 0.  --dry-run keeps the ranks on
the CPU (gloo) and exercises rendezvous, the library's scene partition and a gather shaped like the sweep's."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_rccl_block_and_rank_files(out, rank_dir, world):
    """the line says which RCCL the library bound and how many librccl files the process maps; every rank left
    its own file BEFORE the gather (what a hung collective would leave behind)."""
    r = out["rccl"]
    assert set(r) >= {"amk_shard_bound", "torch_nccl_version", "librccl_files_mapped", "single_rccl_instance"}
    b = r["amk_shard_bound"]
    if b is not None:   # (a box without any librccl: the library reports AMK_ERR_UNSUPPORTED and the block says None)
        assert os.path.basename(b["path"]).startswith("librccl") and b["version"] >= 0
        # torch is imported in the same process: its bundled RCCL was there first and is the one that must have been bound
        assert r["librccl_files_mapped"] is None or b["path"] in r["librccl_files_mapped"] or \
            os.path.realpath(b["path"]) in [os.path.realpath(x) for x in r["librccl_files_mapped"]]
        assert r["single_rccl_instance"] in (True, None), r
    files = sorted(os.listdir(rank_dir))
    assert files == [f"rank{i}.json" for i in range(world)], files
    for i, f in enumerate(files):
        d = json.load(open(os.path.join(rank_dir, f)))
        assert d["rank"] == i and d["world"] == world and d["stage"] == "before the gather" and "rccl" in d


def _run(extra, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "3", "--warmup", "1"] + extra,
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_invocation_spawns_its_ranks(tmp_path):
    out = _run(["--gpus", "2", "--scenes", "5"], {"AMK_BENCH_RANK_DIR": str(tmp_path)})
    assert out["n_gpus"] == 2 and out["ranks_seen"] == 2 and out["gather_ok"] and out["dry_run"]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["scenes_per_rank"] == 5
    _check_rccl_block_and_rank_files(out, str(tmp_path), 2)


def test_single_rank_needs_no_launcher():
    out = _run(["--gpus", "1"])
    assert out["n_gpus"] == 1 and out["gather_ok"]


def test_under_a_launcher_the_world_size_wins(tmp_path):
    """The driver's own command line (`python -m torch.distributed.run ... bench.py --gpus N`): bench.py must not spawn again."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["AMK_BENCH_RANK_DIR"] = str(tmp_path)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr", "127.0.0.1",
                        "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "3", "--dry-run", "--steps", "2",
                        "--scenes", "7"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 3 and out["gather_ok"] and out["padded_scenes_per_rank"] == 7
    _check_rccl_block_and_rank_files(out, str(tmp_path), 3)


def test_dump_outputs_keeps_a_seeded_sample_within_the_byte_budget(tmp_path, monkeypatch):
    """--dump-outputs above its byte budget: the same seeded sample of scenes (and their indices) on every call, all float64."""
    import numpy as np
    import bench
    rng = np.random.default_rng(3)
    outputs = {"u": rng.standard_normal((1000, 4)), "flags": rng.integers(0, 9, (1000, 4)).astype(np.int32)}
    bench.dump_outputs(str(tmp_path / "all"), outputs)
    assert np.array_equal(np.load(tmp_path / "all" / "flags.npy"), outputs["flags"])
    assert not (tmp_path / "all" / "scene_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 20000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outputs)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("u", "flags", "scene_index")}
    assert sum(a.nbytes for a in got.values()) <= 20000 and all(a.dtype == np.float64 for a in got.values())
    idx = got["scene_index"].astype(int)
    assert len(idx) == len(got["u"]) > 100 and np.all(np.diff(idx) > 0)
    assert np.array_equal(got["u"], outputs["u"][idx]) and np.array_equal(got["flags"], outputs["flags"][idx])
    for n in got:
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))
