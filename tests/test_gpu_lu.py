"""The LU direct local solve on the GPU: schwz_trs_create_lu on every dispatch path (one workgroup,
lane-per-row flag sweep, wave-per-row flag sweep, level plan), non-symmetric RAS runs with
--local_factorization=umfpack, parity with the LL^T direct path on symmetric problems, and the
C++ mirror under the reference driver."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
BIN = os.path.join(ROOT, "schwarz-lib_amd", "build", "bench_ras")
MPIEXEC = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"


def _csr(rp, col, val):
    import scipy.sparse as sp
    n = len(rp) - 1
    return sp.csr_matrix((np.asarray(val, dtype=np.float64), np.asarray(col), np.asarray(rp)), shape=(n, n))


def _arrays(A):
    A = A.tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def _shifted_convdiff(convdiff, n):
    import scipy.sparse as sp
    a = _csr(*convdiff(n))
    b = sp.csr_matrix(a[np.roll(np.arange(a.shape[0]), 2), :])
    assert np.all(b.diagonal() == 0.0)
    return _arrays(b)


def _random_blocks(nblocks, seed=7):
    """nblocks independent 5 x 5 blocks, each a well-conditioned diagonally dominant block with
    its rows shuffled (so its diagonal is small and pivoting must move rows), the whole matrix
    symmetrically permuted at random."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    b = 5
    blocks = rng.uniform(-1.0, 1.0, (nblocks, b, b)) * 0.2 + np.eye(b) * rng.uniform(1.0, 2.0, (nblocks, 1, b))
    for k in range(nblocks):
        blocks[k] = blocks[k][rng.permutation(b)]
    rows = (np.arange(nblocks)[:, None, None] * b + np.arange(b)[None, :, None]).repeat(b, axis=2)
    cols = (np.arange(nblocks)[:, None, None] * b + np.arange(b)[None, None, :]).repeat(b, axis=1)
    n = nblocks * b
    A = sp.csr_matrix((blocks.ravel(), (rows.ravel(), cols.ravel())), shape=(n, n))
    p = rng.permutation(n)
    return _arrays(A[p, :][:, p])


def _device_solves(schwz, torch, rp, col, val, natural):
    import scipy.sparse.linalg as sl
    A = _csr(rp, col, val)
    n = A.shape[0]
    f = schwz.lu(rp, col, val, natural=natural)
    t = schwz.TrsLU(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"], f["row_perm"],
                    f["col_perm"])
    rng = np.random.default_rng(11)
    Ac = A.tocsc()
    for _ in range(2):  # twice: the flag vectors must come back reset
        b = rng.standard_normal(n)
        d_b = torch.tensor(b, device="cuda", dtype=torch.float64)
        d_y = torch.full((n,), float("nan"), device="cuda", dtype=torch.float64)
        t.solve(d_b.data_ptr(), d_y.data_ptr())
        torch.cuda.synchronize()
        y = d_y.cpu().numpy()
        x = sl.spsolve(Ac, b)
        assert np.isfinite(y).all()
        assert np.abs(y - x).max() <= 1e-12 * np.abs(x).max()
    t.close()
    return f


def _longest(f):
    return max(np.diff(f["l_rp"]).max(), np.diff(f["u_rp"]).max())


def test_lu_trs_one_workgroup(schwz, torch_cuda, convdiff):
    f = _device_solves(schwz, torch_cuda, *_shifted_convdiff(convdiff, 20), natural=False)
    assert not np.array_equal(f["row_perm"], f["col_perm"])


def test_lu_trs_lane_flag_sweep(schwz, torch_cuda):
    rp, col, val = _random_blocks(12000)
    f = _device_solves(schwz, torch_cuda, rp, col, val, natural=True)
    assert len(rp) - 1 > 8192 and _longest(f) <= 5
    assert not np.array_equal(f["row_perm"], f["col_perm"])


@pytest.mark.parametrize("flags", ["1", "0"])  # 0: the level-by-level launch plan
def test_lu_trs_long_rows(schwz, torch_cuda, convdiff, monkeypatch, flags):
    monkeypatch.setenv("SCHWZ_TRS_FLAGS", flags)
    rp, col, val = convdiff(128)
    f = _device_solves(schwz, torch_cuda, rp, col, val, natural=False)
    assert len(rp) - 1 == 16384 and _longest(f) > 64


def _run_gpu(schwz, P, settings_kw, metadata_kw):
    s = schwz.Settings(**settings_kw)
    m = schwz.Metadata(num_subdomains=P, **metadata_kw)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    out = solver.run()
    return solver, m, out


def _write_mtx(path, rp, col, val):
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, rp[-1]))
        for r, c, v in zip(rows, col, val):
            f.write("%d %d %.17g\n" % (r + 1, c + 1, v))
    return path


def _gmres_exact_reference(oracle, rp, col, val, P, m):
    """The oracle's RAS with GMRES local solves that are exact to rounding (Krylov space = the local
    system)."""
    N = len(rp) - 1
    return oracle.ras_run(rp, col, val, np.ones(N), P, np.asarray(m.first_row, dtype=np.int32),
                          oracle.make_settings(max_iters=m.max_iters, tol=m.tolerance, local_tol=1e-14,
                                               local_max_iters=N, non_symmetric=1, restart_iter=N))


@pytest.mark.parametrize("P", [1, 4])
def test_ras_non_symmetric_direct_lu(schwz, oracle, torch_cuda, convdiff, tmp_path, P):
    import scipy.sparse.linalg as sl
    rp, col, val = convdiff(30)
    n = len(rp) - 1
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    solver, m, out = _run_gpu(
        schwz, P, dict(matrix_filename=path, explicit_laplacian=False, non_symmetric_matrix=True,
                       local_solver="direct-ginkgo", factorization="umfpack"),
        dict(tolerance=1e-8, max_iters=400))
    r = _gmres_exact_reference(oracle, rp, col, val, P, m)
    x = sl.spsolve(_csr(rp, col, val).tocsc(), np.ones(n))
    assert out["converged"] and r["converged"]
    assert abs(out["iter_count"] - r["iter_count"]) <= 1
    assert np.abs(out["solution"] - x).max() <= 1e-8 * np.abs(x).max()


def _parity_with_ll_t(oracle, csr, P, m, solver, out):
    rp, col, val = csr
    N = len(rp) - 1
    s = solver.settings
    r = oracle.ras_run(rp, col, val, np.ones(N), P, np.asarray(m.first_row, dtype=np.int32),
                       oracle.make_settings(max_iters=m.max_iters, tol=m.tolerance, overlap=s.overlap,
                                            local_solver=oracle.SOLVER_DIRECT,
                                            natural_factor_ordering=int(s.naturally_ordered_factor)))
    assert out["converged"] and r["converged"]
    hist = np.array(m.post_process_data["global_residual_vector_out"]).sum(axis=0)
    g0 = r["hist_global"][0]
    if out["iter_count"] != r["iter_count"]:
        # a stop decided by rounding: only when the oracle's last residual sits at the tolerance
        assert abs(out["iter_count"] - r["iter_count"]) == 1
        last = r["hist_global"][-1]
        assert abs(last - m.tolerance * g0) <= 1e-6 * m.tolerance * g0
    k = min(len(hist), len(r["hist_global"]))
    assert np.abs(hist[:k] - r["hist_global"][:k]).max() <= 1e-9 * g0
    scale = np.abs(r["solution"]).max()
    assert np.abs(out["solution"] - r["solution"]).max() <= 1e-8 * scale


def test_lu_matches_ll_t_on_lap2d(schwz, oracle, torch_cuda):
    n, P = 32, 4
    solver, m, out = _run_gpu(schwz, P, dict(local_solver="direct-ginkgo", factorization="umfpack"),
                              dict(oned_laplacian_size=n, tolerance=1e-8, max_iters=300))
    _parity_with_ll_t(oracle, oracle.laplacian2d(n), P, m, solver, out)


def test_lu_matches_ll_t_on_ani4_eight_subdomains(schwz, oracle, torch_cuda, tmp_path):
    g = np.load(os.path.join(G, "ani4_crop.npz"))
    path = _write_mtx(str(tmp_path / "a.mtx"), g["rp"], g["col"], g["val"])
    solver, m, out = _run_gpu(
        schwz, 8, dict(matrix_filename=path, explicit_laplacian=False, local_solver="direct-ginkgo",
                       factorization="umfpack"),
        dict(tolerance=1e-8, max_iters=3000))
    _parity_with_ll_t(oracle, (g["rp"], g["col"], g["val"]), 8, m, solver, out)


def test_debug_dumps_of_the_lu(schwz, torch_cuda, convdiff, tmp_path, monkeypatch):
    rp, col, val = convdiff(12)
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    monkeypatch.chdir(tmp_path)
    solver, m, out = _run_gpu(
        schwz, 2, dict(matrix_filename=path, explicit_laplacian=False, non_symmetric_matrix=True,
                       local_solver="direct-ginkgo", factorization="umfpack", write_perm_data=True,
                       print_matrices=True),
        dict(tolerance=1e-8, max_iters=200))
    assert out["converged"]
    for me, sd in solver.subdomains.items():
        lrp, lcol, lval = sd.local_matrix()
        f = schwz.lu(lrp, lcol, lval)
        perm = np.loadtxt(tmp_path / ("perm_%d.csv" % me), dtype=np.int64)
        inv = np.loadtxt(tmp_path / ("inv_perm_%d.csv" % me), dtype=np.int64)
        assert np.array_equal(perm, f["row_perm"])
        assert np.array_equal(inv[f["col_perm"]], np.arange(len(inv)))
        assert (tmp_path / ("L_mat_%d.csv" % me)).exists() and (tmp_path / ("U_mat_%d.csv" % me)).exists()


def test_bench_ras_direct_lu_non_symmetric(schwz, convdiff, tmp_path):
    """The reference driver, unchanged: --local_solver=direct-ginkgo --local_factorization=umfpack
    --non_symmetric_matrix on two ranks; same iteration count as the Python host."""
    if not os.path.exists(BIN):
        pytest.skip("bench_ras binary not built (needs the reference checkout at build time)")
    if not os.path.exists(MPIEXEC):
        pytest.skip("no mpiexec on this machine")
    rp, col, val = convdiff(26)
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    cmd = [MPIEXEC, "-n", "2", BIN, "--executor=hip", "--matrix_filename=%s" % path, "--enable_global_check",
           "--num_iters=500", "--set_tol=1e-8", "--non_symmetric_matrix", "--local_solver=direct-ginkgo",
           "--local_factorization=umfpack", "--write_perm_data"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    iters = sorted(set(int(x) for x in re.findall(r"converged in (\d+) iterations", p.stdout)))
    solver, m, out = _run_gpu(
        schwz, 2, dict(matrix_filename=path, explicit_laplacian=False, non_symmetric_matrix=True,
                       local_solver="direct-ginkgo", factorization="umfpack"),
        dict(tolerance=1e-8, max_iters=500))
    assert out["converged"] and iters == [out["iter_count"]], p.stdout
    for me in range(2):
        for name in ("perm_%d.csv", "inv_perm_%d.csv"):
            v = np.loadtxt(tmp_path / (name % me), dtype=np.int64)
            assert np.array_equal(np.sort(v), np.arange(len(v)))
