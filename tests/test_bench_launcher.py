"""`python bench.py --gpus N` must itself run N ranks: the launcher path, the rendezvous and a collective,
on CPU with gloo (CXRK_BENCH_SELFTEST=1 skips the GPU work; everything else is the code the real run takes)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_cmd_is_one_rank_per_gpu_on_localhost():
    sys.path.insert(0, ROOT)
    import bench
    cmd = bench.launch_cmd(4, ["--gpus", "4", "--steps", "3"], 29511)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29511"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and cmd[-5].endswith("bench.py")


def test_plain_command_spawns_the_ranks_and_fails_loudly():
    env = dict(os.environ, CXRK_BENCH_SELFTEST="1", CXRK_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["rccl_ranks"] == 2 and out["n_gpus"] == 2
    # a rank that dies makes the plain command exit non-zero (never a silent one-GPU measurement)
    env["CXRK_DIST_BACKEND"] = "no-such-backend"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0


def test_plain_run_times_the_steps_only_and_full_restores_the_rest():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, None)
    assert a.no_secondary and a.no_roofline and a.no_cpu_baseline
    f = bench.parse(["--full"])
    assert f.full and not (f.no_secondary or f.no_roofline or f.no_cpu_baseline)
    g = bench.parse(["--full", "--no-cpu-baseline", "--dump-outputs", "out"])
    assert g.no_cpu_baseline and not g.no_secondary and g.dump_outputs == "out"


def test_dump_outputs_writes_a_fixed_float32_sample_within_budget(tmp_path):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    assert 2 * bench.DUMP_SAMPLE * 4 + 4 <= 64 << 20                  # params + grads samples + loss, float32
    n = 3 * bench.DUMP_SAMPLE
    flat_p = torch.arange(n, dtype=torch.float32)
    flat_g = -torch.arange(n, dtype=torch.float32) / n
    shapes = bench.dump_outputs(str(tmp_path / "a"), torch.tensor(6.93), flat_p, flat_g)
    bench.dump_outputs(str(tmp_path / "b"), torch.tensor(6.93), flat_p, flat_g)
    assert shapes == {"loss": [1], "params_sample": [bench.DUMP_SAMPLE], "grads_sample": [bench.DUMP_SAMPLE]}
    for name in shapes:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)        # same positions in every run
    p = np.load(tmp_path / "a" / "params_sample.npy")
    g = np.load(tmp_path / "a" / "grads_sample.npy")
    assert np.all(np.diff(p) >= 0) and p.max() > 0.9 * n              # spread over the whole buffer
    np.testing.assert_array_equal(g, -p / n)                          # gradient sampled at the parameters' positions
    assert np.load(tmp_path / "a" / "loss.npy")[0] == np.float32(6.93)
