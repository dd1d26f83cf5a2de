"""The bench lines committed under profiles/ carry every field of the driver contract (bench.py writes them; this guards the
contract against accidental edits -- it does not run the bench)."""
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def _check_roofline(r):
    assert r["bound"] in ("hbm", "mfma") and r["unit"] == {"hbm": "GB/s", "mfma": "TFLOP/s"}[r["bound"]]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["kernel_avg_us"] > 0
    if r["bound"] == "hbm":
        assert r["peak"] == 8000.0
        assert r["traffic"] is None or r["traffic"] >= 0.9 * r["algorithmic_bytes_per_launch"]
    else:
        assert r["peak"] == 2500.0                 # the ISSUED 16-bit MFMA products (2-3 per f32-equivalent product) against the dense f16/bf16 peak
        assert r["algorithmic_flops_per_launch"] > 0
        a32 = r.get("algorithmic_f32")      # informational second pricing: the reference's f32 FLOPs against the f32-MFMA peak
        assert a32 is None or (a32["peak"] == 157.3 and abs(a32["frac"] - a32["achieved"] / a32["peak"]) < 1e-9
                               and a32["algorithmic_flops_per_launch"] <= r["algorithmic_flops_per_launch"])


@pytest.mark.parametrize("name", ["r02_bench_e2e_cleanup5.json", "r02_bench_e2e_harvest5.json", "r02_bench_e2e_cleanup10.json",
                                  "r02_bench_env_cleanup5.json", "r03_bench_e2e_cleanup5.json", "r03_bench_e2e_harvest5.json",
                                  "r03_bench_e2e_cleanup10.json", "r03_bench_env_cleanup5.json", "r03_bench_e2e_cleanup5_tspr8.json",
                                  "r04_bench_e2e_cleanup5.json", "r04_bench_e2e_harvest5.json", "r04_bench_e2e_cleanup10.json", "r04_bench_env_cleanup5.json",
                                  "r04_bench_e2e_cleanup5_tspr8.json", "r04_bench_e2e_cleanup5_learner_bf16_tspr8.json"])
def test_committed_bench_line_has_the_contract_fields(name):
    d = json.load(open(os.path.join(ROOT, "profiles", name)))
    for k in REQUIRED:
        assert k in d or (k == "cpu_baseline" and ("r02_bench_env" in name or "tspr8" in name)), k      # lines taken with --no-cpu-baseline
    assert d["metric"] == "agent_steps_per_sec" and d["unit"] == "agent-steps/s" and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    _check_roofline(d["roofline"])
    for k in d.get("kernels", []):
        _check_roofline(k)
    assert d["roofline"]["kernel_avg_us"] == max(k["kernel_avg_us"] for k in d.get("kernels", [d["roofline"]]))      # the DOMINANT kernel is the one reported
    cfg = d["config"]
    assert cfg["world_size"] == d["n_gpus"] and cfg["backend"]
    units = cfg["n_env_per_gpu"] * cfg["n_agents"] * d["n_gpus"] * d["steps"]
    if "e2e" in name:       # one e2e step = one whole iteration: a 100-timestep rollout of every env + the train steps
        units *= cfg["episode_limit"]
        assert cfg["timesteps_timed"] == d["steps"] * cfg["episode_limit"] and cfg["train_steps_timed"] >= d["steps"]
    assert abs(d["value"] - units / (d["ms_per_step"] * d["steps"] / 1e3)) < 1e-3 * d["value"]
    ew = d.get("env_workload")      # round 4: the format-R env workload measured after the timed region of the e2e line (1 GPU)
    if name.startswith("r04_bench_e2e") and d["n_gpus"] == 1:
        assert ew is not None and ew["unit"] == "GB/s" and ew["peak"] == 8000.0 and abs(ew["frac"] - ew["achieved"] / ew["peak"]) < 1e-9
        assert abs(ew["achieved"] - ew["algorithmic_bytes_per_launch"] / (ew["avg_us"] * 1e-6) / 1e9) < 1e-6 * ew["achieved"] and ew["transitions"] >= 100
    c = d.get("cpu_baseline")
    assert c is None or c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["unit"] == "agent-steps/s" and c["sample"]


def test_roofline_bytes_follow_the_survey_formula():
    import sys
    sys.path.insert(0, ROOT)
    from bench import algorithmic_bytes_per_env_step
    assert algorithmic_bytes_per_env_step(25, 18, 5, 15) == 14640       # Cleanup-5, SURVEY.md section 8(d)
    assert algorithmic_bytes_per_env_step(10, 10, 3, 15) == 8444        # Cleanup-3
    assert algorithmic_bytes_per_env_step(48, 18, 10, 15) == 29208      # Cleanup-10
    assert algorithmic_bytes_per_env_step(9, 38, 5, 31) == 58584        # Harvest-5


def test_bench_front_door_starts_its_own_ranks_for_n_gt_1():
    """`python bench.py --gpus 2` with no launcher around it (the driver's command form) starts two ranks as a child
    torch.distributed.run job, the ranks count each other with an all-reduce, and exactly one JSON line comes back on stdout."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-dry-run"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["ranks_seen"] == 2 and d["config"]["world_size"] == 2 and d["config"]["self_launched"] is True


def test_bench_front_door_propagates_a_failing_rank():
    """a rank that dies makes the self-launched job exit non-zero and print no JSON line."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SSD_DRY_RUN_FAIL_RANK"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-dry-run"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode != 0 and not p.stdout.decode().strip()


def test_dump_outputs_writes_a_fixed_float_sample_within_the_budget(tmp_path):
    """--dump-outputs: float32 / float64 files only (float64 where float32 would round), at most 64 MB on disk, and when the per-env
    outputs do not fit, the same seeded sample of envs in every run and in every per-env array."""
    import sys
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    N = 4096
    code = torch.arange(N, dtype=torch.uint8).view(N, 1, 1, 1).expand(N, 101, 5, 225)      # 465 MB as f32: must be sampled
    ids = (torch.arange(N, dtype=torch.int64) * 1000003).view(N, 1)                          # beyond f32's exact integers
    w = torch.randn(64, 9, dtype=torch.float32)
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        files, nbytes = bench.dump_outputs(str(d), {"obs": code, "ids": ids}, {"param.w": w}, N)
        assert files == 4 and nbytes <= bench.DUMP_BUDGET_BYTES
        assert sum(f.stat().st_size for f in d.iterdir()) == nbytes
        out = {f.name[:-4]: np.load(f) for f in d.iterdir()}
        assert sorted(out) == ["env_index", "ids", "obs", "param.w"]
        assert out["obs"].dtype == np.float32 and out["param.w"].dtype == np.float32
        assert out["ids"].dtype == np.float64 and out["env_index"].dtype == np.float64
        sel = out["env_index"].astype(np.int64)
        assert 0 < len(sel) < N and (np.diff(sel) > 0).all()
        assert (out["obs"] == (sel % 256).reshape(-1, 1, 1, 1)).all() and (out["ids"][:, 0] == sel * 1000003).all()
        assert (out["param.w"] == w.numpy()).all()
        runs.append(sel)
    assert (runs[0] == runs[1]).all()
    # outputs that fit are written whole, without an index
    d = tmp_path / "whole"
    assert bench.dump_outputs(str(d), {"reward": torch.ones(N, 5)}, {}, N)[0] == 1
    assert np.load(d / "reward.npy").shape == (N, 5)


def test_bench_has_the_full_and_dump_outputs_options():
    """the plain run and the --full run share one front door: both options parse without touching the GPU"""
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and "--full" in p.stdout.decode() and "--dump-outputs" in p.stdout.decode()


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["e2e", "env"])
def test_plain_bench_run_times_its_steps_and_dumps_its_outputs(workload, tmp_path):
    """A plain run: exactly --steps timed steps, the headline fields, none of the --full measurements, and the last timed step's
    outputs under --dump-outputs (float32 / float64, at most 64 MB)."""
    import subprocess
    import sys
    import numpy as np
    steps = 3 if workload == "e2e" else 50
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--workload", workload, "--dump-outputs", str(tmp_path)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"] == "agent_steps_per_sec" and d["unit"] == "agent-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] in ("fp32", "u8") and d["steps"] == steps and d["ms_per_step"] > 0
    for k in ("roofline", "kernels", "cpu_baseline", "env_workload"):
        assert k not in d, k
    assert "breakdown_ms" not in d["config"]
    cfg = d["config"]
    units = cfg["n_env_per_gpu"] * cfg["n_agents"] * steps * (cfg["episode_limit"] if workload == "e2e" else 1)
    assert abs(d["value"] - units / (d["ms_per_step"] * steps / 1e3)) < 1e-3 * d["value"]
    if workload == "e2e":
        assert cfg["timesteps_timed"] == steps * cfg["episode_limit"] and cfg["rollouts_timed"] == steps
    files = {f.name[:-4]: f for f in tmp_path.iterdir()}
    assert sum(f.stat().st_size for f in files.values()) <= 64 * 10 ** 6
    assert "reward" in files and "obs" in files
    if workload == "e2e":
        assert "train_logs" in files and any(k.startswith("param.") for k in files)
    for f in files.values():
        a = np.load(f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f.name
