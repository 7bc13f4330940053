"""Two-level RAS through the C++ mirror (Metadata::coarse_space / coarse_aggregates / coarse_aggregate_vector of
schwarz-lib_amd/host): tests/drivers/coarse_driver.cpp under mpiexec, three ranks sharing this GPU, against the Python
host's in-process run of the same case -- the 12 x 12 x 12 Laplacian in 3 z-slabs, direct local solves, 4 x 4 x 2 boxes
(54 aggregates).  Iteration counts equal, residual histories to 1e-12 G0."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "schwarz-lib_amd", "build", "coarse_driver")
MPIEXEC = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"


def _driver(nranks, *args):
    if not os.path.exists(DRIVER):
        pytest.skip("coarse_driver not built (`make -C schwarz-lib_amd coarse_driver`, needs MPI)")
    if not os.path.exists(MPIEXEC):
        pytest.skip("no mpiexec on this machine")
    cmd = [MPIEXEC, "-n", str(nranks), DRIVER] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def _python_host(schwz, P, n, **coarse):
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(n, n, n), local_solver="direct-ginkgo", overlap=2)
    m = schwz.Metadata(num_subdomains=P, tolerance=1e-8, max_iters=200, **coarse)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    out = solver.run()
    return out, np.array(m.post_process_data["global_residual_vector_out"]).sum(axis=0)


def _boxes(n, bx, by, bz):
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    cx, cy = -(-n // bx), -(-n // by)
    return (((z // bz) * cy + y // by) * cx + x // bx).reshape(-1).astype(np.int64)


@pytest.mark.parametrize("mode", ["vector", "automatic", "none"])
def test_mirror_runs_the_two_level_iteration_like_the_python_host(schwz, torch_cuda, mode):
    P, n = 3, 12
    if mode == "vector":
        p = _driver(P, "aggregates", n, 4, 4, 2, 1e-8, 200)
        coarse = dict(coarse_space="aggregates", coarse_aggregate_vector=_boxes(n, 4, 4, 2))
    elif mode == "automatic":
        p = _driver(P, "aggregates", n, 0, 0, 0, 1e-8, 200, "auto", 6)
        coarse = dict(coarse_space="aggregates", coarse_aggregates=6)
    else:
        p = _driver(P, "none", n, 4, 4, 2, 1e-8, 200)
        coarse = dict()
    assert p.returncode == 0, p.stdout + p.stderr
    res = re.search(r"RESULT iters=(\d+)", p.stdout)
    hist = re.search(r"^HIST (.*)$", p.stdout, re.M)
    assert res and hist, p.stdout
    said = re.search(r"Two-level RAS: (\d+) aggregates", p.stdout)
    assert (said is not None) == (mode != "none")
    if mode == "vector":
        assert int(said.group(1)) == 54
    got = np.array([float(v) for v in hist.group(1).split()])
    out, want = _python_host(schwz, P, n, **coarse)
    print("%s: mirror %s iterations, python host %d" % (mode, res.group(1), out["iter_count"]))
    assert out["converged"] and int(res.group(1)) == out["iter_count"]
    assert len(got) == len(want)
    assert np.abs(got - want).max() <= 1e-12 * want[0]


def test_mirror_refuses_an_unknown_coarse_space():
    p = _driver(1, "boxes", 8, 4, 4, 4, 1e-8, 10)
    assert p.returncode == 3, p.stdout + p.stderr
    assert "REFUSED" in p.stdout
