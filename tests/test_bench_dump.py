"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy files, within the size cap."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN_ENV = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _run_bench(args, timeout):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=CLEAN_ENV, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones_the_same_way(tmp_path):
    bench = _bench_module()
    rng = np.random.default_rng(3)
    arrays = {"big": rng.random(200_000), "mid": rng.random((40, 50)), "small": np.arange(5.0)}
    cap = 1 << 20
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, cap=cap)
    a, b = _load_dir(tmp_path / "a"), _load_dir(tmp_path / "b")
    assert sorted(a) == ["big", "mid", "small"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= cap
    assert np.array_equal(a["small"], arrays["small"]) and np.array_equal(a["mid"], arrays["mid"])
    assert 0 < a["big"].size < arrays["big"].size and np.isin(a["big"], arrays["big"]).all()
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k])
    bench.dump_outputs(str(tmp_path / "c"), {"small": arrays["small"]})          # under the cap: written as computed
    assert np.array_equal(np.load(tmp_path / "c" / "small.npy"), arrays["small"])


def test_stub_bench_dumps_the_last_steps_costs(tmp_path):
    r = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--stub-solver", "--dump-outputs", str(tmp_path)], 120)
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert _load_dir(tmp_path) == {"costs_all_ranks": np.array([r["cost"]])}


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_timed_paths_and_repeat(tmp_path):
    small = ["--gpus", "1", "--warmup", "1", "--roofline-cells", "0", "--cpu-sample", "0", "--pgd-iters", "0", "--batched=",
             "--systems", "0"]
    r2 = _run_bench(small + ["--steps", "2", "--dump-outputs", str(tmp_path / "s2")], 300)
    r3 = _run_bench(small + ["--steps", "3", "--dump-outputs", str(tmp_path / "s3")], 300)
    assert r2["steps"] == 2 and r3["steps"] == 3 and r2["ms_per_step"] > 0
    o2, o3 = _load_dir(tmp_path / "s2"), _load_dir(tmp_path / "s3")
    n, Nt = r2["config"]["nodes"], r2["config"]["num_steps"]
    assert sorted(o2) == ["adjoint_p", "cost", "costs_all_ranks", "descent_d", "state_u"]
    assert o2["state_u"].shape == o2["adjoint_p"].shape == (1, Nt + 1, n) and o2["descent_d"].shape == (Nt + 1, n)
    assert o2["cost"][0] == r2["cost"] and o2["costs_all_ranks"][0] == r2["cost"]
    assert np.array_equal(o2["state_u"][0, 0], _bench_module().slotted_disc_ic(-1.0, 1.0, 0.025))   # level 0 = the input IC
    for k in o2:
        assert np.isfinite(o2[k]).all()
        np.testing.assert_allclose(o3[k], o2[k], rtol=1e-12, atol=1e-14, err_msg=k)   # same inputs, same outputs


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_and_full_adds_the_sub_benchmarks():
    extras = {"kernels_c2", "roofline", "batched", "systems", "small_mesh_batches", "pgd_c2", "pgd_c5_mixed_decisions",
              "cpu_baseline", "parity", "tolerance_table"}
    plain = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1"], 300)
    assert plain["steps"] == 2 and plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["cost"] > 0
    assert plain["metric"] == "FCT timesteps/sec (fwd+adj)" and plain["unit"] == "timesteps/s" and plain["dtype"] == "f64"
    assert plain["higher_is_better"] is True and len(plain["config"]["source_sha16"]) == 16
    assert not extras & set(plain), sorted(extras & set(plain))
    full = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--roofline-cells", "0", "--cpu-sample", "0",
                       "--pgd-iters", "0", "--batched=", "--systems", "0"], 300)
    assert full["kernels_c2"] and all(e["launches_per_sweep"] > 0 for e in full["kernels_c2"].values())
    assert not (extras - {"kernels_c2"}) & set(full)                      # the others were switched off one by one
    assert abs(full["cost"] - plain["cost"]) <= 1e-12 * plain["cost"]    # same inputs, same timed path
