"""CPU: bench.py starts its own ranks when asked for N > 1 GPUs without a launcher (child process of
``python -m torch.distributed.run``, started before anything touches the GPU), refuses a WORLD_SIZE that contradicts
--gpus, and the BASELINE config presets resolve.  ``--dry-run`` = rank start-up + barrier only (gloo here)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["RATO_DIST_BACKEND"] = "gloo"
    return env


def test_bench_spawns_its_own_ranks():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], env=_env(), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout                      # ONE JSON line, from rank 0
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["dry_run"] is True


def test_bench_refuses_contradicting_world_size():
    env = _env()
    env.update(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], env=env, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2 and "WORLD_SIZE=3" in out.stderr


def test_config_presets():
    sys.path.insert(0, ROOT)
    import bench
    argv = sys.argv
    try:
        for cfg, want in (("metric", ("drone", 100000, 50)), ("C2", ("drone", 10000, 50)),
                          ("C3", ("driving", 10000, 40)), ("C4", ("hopper", 50000, 60)), ("C5", ("driving", 125000, 40))):
            sys.argv = ["bench.py", "--config", cfg]
            a = bench.parse()
            assert (a.workload, a.M, a.S) == want
        sys.argv = ["bench.py", "--config", "C5", "--M", "1000"]
        a = bench.parse()
        assert (a.workload, a.M, a.S) == ("driving", 1000, 40)
    finally:
        sys.argv = argv


def test_bench_eight_ranks_dry_run_c5():
    """the launch path of `bench.py --gpus 8 --config C5` (BASELINE C5: driving, M = 1e6 over 8 GPUs): eight ranks come
    up (gloo here), LOCAL_RANK -> device, 125,000 samples per GPU, M_total = 1,000,000, ONE line from rank 0"""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--config", "C5", "--dry-run", "--strict-comm"],
                         env=_env(), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    cfg = line["config"]
    assert line["n_gpus"] == 8 and line["scaling"] == "weak"
    assert (cfg["workload"], cfg["M_per_gpu"], cfg["S"], cfg["M_total"]) == ("driving", 125000, 40, 1000000)
    assert [r["device"] for r in sorted(cfg["ranks"], key=lambda r: r["rank"])] == [f"cuda:{i}" for i in range(8)]
    assert cfg["strict_comm"] is True


def test_full_and_dump_options():
    """a plain run times the products Jacobian alone; --full restores every representation (and the side blocks)"""
    sys.path.insert(0, ROOT)
    import bench
    argv = sys.argv
    try:
        for extra, jac in (([], "products"), (["--full"], "both"), (["--full", "--jacobian", "factored"], "factored")):
            sys.argv = ["bench.py", "--steps", "7"] + extra
            a = bench.parse()
            assert a.jacobian == jac and a.full == ("--full" in extra) and a.steps == 7 and a.dump_outputs is None
        sys.argv = ["bench.py", "--dump-outputs", "out"]
        assert bench.parse().dump_outputs == "out"
    finally:
        sys.argv = argv


def test_collect_outputs_samples_and_untiles():
    """--dump-outputs: G [n_tiles][n_pairs][2][n_obs][tile] comes back untiled for a fixed sorted sample of the samples;
    per-sample arrays above DUMP_FULL_BYTES keep the same sample, the small ones are whole; float32 / float64 only"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    M, S, tile, n_pairs = 5000, 8, 64, 28
    n_tiles = (M + tile - 1) // tile
    sample = torch.arange(n_tiles * tile, dtype=torch.float32).reshape(n_tiles, 1, 1, 1, tile)
    G = sample + 1e5 * torch.arange(n_pairs * 6, dtype=torch.float32).reshape(1, n_pairs, 2, 3, 1)
    g_up = torch.arange(3 * S * 1, dtype=torch.float32).reshape(3, S, 1) * 1e5 + torch.arange(M, dtype=torch.float32)
    big = torch.arange(M, dtype=torch.float32).repeat(300, 1)                     # 6 MB: sampled
    r = {"G": G, "g_up": g_up, "Z": torch.arange(M, dtype=torch.float32), "tile": tile}

    class Work:
        pass
    w = Work()
    w.M = M
    w.outputs = lambda r_, sums: {"G": r_["G"], "g_up": r_["g_up"], "Z": r_["Z"], "big": big, "sums": sums, "none": None}
    out = bench.collect_outputs(w, r, torch.arange(6, dtype=torch.float64), torch.arange(11, dtype=torch.float64))
    idx = np.sort(np.random.RandomState(0).choice(M, 1024, replace=False))
    assert sorted(out) == ["G", "Z", "big", "g_up", "stats", "sums"]
    assert out["G"].shape == (n_pairs, 2, 3, 1024) and out["G"].dtype == np.float32
    np.testing.assert_array_equal(out["G"] % 1e5, np.broadcast_to(idx, (n_pairs, 2, 3, 1024)))
    np.testing.assert_array_equal(out["G"][:, :, :, 0] // 1e5, np.arange(n_pairs * 6).reshape(n_pairs, 2, 3))
    np.testing.assert_array_equal(out["g_up"], g_up.numpy())                     # 96 KB: whole
    np.testing.assert_array_equal(out["Z"], np.arange(M))
    np.testing.assert_array_equal(out["big"], np.broadcast_to(idx, (300, 1024)))
    assert out["stats"].dtype == np.float64 and out["sums"].dtype == np.float64 and out["stats"].shape == (11,)
