"""bench.py's own launcher: `python bench.py --gpus N` with no launcher around it starts its N
rank processes itself (the driver invokes it exactly like that)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


@pytest.mark.parametrize("n", [2, 4])
def test_self_launch_rendezvous_on_cpu(n):
    """The launcher alone, on CPU: N children with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set,
    a gloo rendezvous on 127.0.0.1 among them, rank 0's line relayed on the parent's stdout,
    exit code 0.  (The GPU work of bench.py is replaced by the probe; the process tree, the
    environment and the relay are the real ones.)"""
    p = subprocess.run([sys.executable, BENCH, "--gpus", str(n)], capture_output=True, text=True, timeout=600,
                       env=_clean_env(SCHWZ_BENCH_LAUNCH_PROBE="1"))
    assert p.returncode == 0, p.stdout + p.stderr
    got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert got["launch_probe"] and got["world"] == n and got["n_gpus"] == n
    assert got["ranks"] == [[r, r] for r in range(n)]


def test_self_launch_reports_a_failing_rank():
    """A rank that dies makes the launcher exit non-zero (here: every rank rejects a bad flag)."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--no-such-flag"], capture_output=True, text=True,
                       timeout=300, env=_clean_env(SCHWZ_BENCH_LAUNCH_PROBE="1"))
    assert p.returncode != 0


def test_self_launch_ends_the_other_ranks_when_one_dies_at_start_up():
    """Rank 1 exits before the rendezvous: rank 0 would wait for it until the process-group timeout.  The
    launcher watches every child, ends the survivors and reports the failing rank's code within seconds."""
    import time
    t0 = time.time()
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True, timeout=240,
                       env=_clean_env(SCHWZ_BENCH_LAUNCH_PROBE="1", SCHWZ_BENCH_PROBE_FAIL_RANK="1"))
    assert p.returncode == 3, p.stdout + p.stderr
    assert time.time() - t0 < 120
    assert "other ranks were stopped" in p.stderr


@pytest.mark.gpu
def test_bench_gpus_2_starts_itself_and_prints_one_line():
    """`python bench.py --gpus 2 --full` as the driver calls it.  On a box with fewer GPUs than
    ranks the two ranks share the GPU and stage halos through host over gloo (the line says so);
    with two GPUs the same command runs on RCCL.  Small slabs: this checks the launch path, the
    distributed branch and the shape of the line, not performance."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1", "--slab", "48,40,16",
                        "--full", "--no-cpu-baseline", "--ttr-budget-s", "20", "--strong-grid", "48,40,32",
                        "--strong-steps", "3"],
                       capture_output=True, text=True, timeout=900, env=_clean_env())
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    got = json.loads(lines[0])
    assert got["n_gpus"] == 2 and got["steps"] == 3 and got["scaling"] == "weak"
    assert got["unit"] == "subdomain-iter/s" and got["value"] > 0
    assert got["config"]["rows_per_gpu"] >= 48 * 40 * 16
    import torch
    backend = got["config"]["exchange_backend"]
    assert backend.startswith("nccl" if torch.cuda.device_count() >= 2 else "gloo")
    assert 0.0 < got["roofline"]["frac"] <= 1.0
    # the strong-scaling leg of the same job: the fixed grid cut into N z-slabs
    assert got["strong"]["grid"] == "48x40x32" and got["strong"]["subdomains"] == 2 and got["strong"]["outer_iter_per_s"] > 0
    assert "mirror_bench_ras" not in got   # the C++ mirror's line belongs to the N = 1 run
    assert got["time_to_residual_converged"] and got["true_relative_residual"] < 1e-4


@pytest.mark.gpu
def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(oracle, tmp_path):
    """A plain run (no --full) prints the headline line only, over exactly --steps timed steps, and
    --dump-outputs writes what the last timed step left: the iterate of the whole grid (the oracle's
    after the same 1 + warmup + steps outer iterations) and the residual history of the warm-up and timed
    steps, the same from run to run."""
    import numpy as np
    n, warmup, steps = 40, 2, 4
    got = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--size", str(n), "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=300, env=_clean_env())
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        line = json.loads(lines[0])
        assert line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
        assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "subdomain-iter/s"
        assert line["dtype"] == "f64" and line["higher_is_better"] is True
        for leg in ("roofline", "roofline_csr_plain", "hbm_measured", "strong", "csr_plain_loop",
                    "time_to_residual_1e-6_s", "cpu_baseline", "mirror_bench_ras"):
            assert leg not in line, leg
        assert sorted(os.listdir(d)) == ["residual_history.npy", "solution.npy"]
        x, h = np.load(d / "solution.npy"), np.load(d / "residual_history.npy")
        assert x.dtype == np.float64 and x.shape == (n ** 3,)
        # the timed run restarts the history after the untimed set-up step; the iterate carries on from it
        assert h.dtype == np.float64 and h.shape == (1, warmup + steps)
        got.append((x, h))
    np.testing.assert_allclose(got[1][0], got[0][0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[1][1], got[0][1], rtol=1e-12, atol=0)
    rp, col, val = oracle.laplacian3d(n, n, n)
    N = len(rp) - 1
    r = oracle.ras_run(rp, col, val, np.ones(N), 1, oracle.first_rows_regular(N, 1),
                       oracle.make_settings(max_iters=1 + warmup + steps, tol=1e-30, precond=oracle.PRECOND_JACOBI,
                                            local_tol=0.0, local_max_iters=10))
    assert r["iter_count"] == 1 + warmup + steps
    x = got[0][0]
    assert np.abs(x - r["solution"]).max() <= 1e-8 * np.abs(r["solution"]).max()
