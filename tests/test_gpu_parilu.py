"""ParILU factors and Jacobi-sweep triangular solves on the GPU (schwz_parilu, schwz_trs_create_sweeps,
Metadata.par_ilu_sweeps / trisolve_sweeps): against numpy restatements of the synchronous sweeps and of the
truncated Neumann series, against the exact ILU(0) and exact solves once the sweep counts cover the
dependency chains, inside CG / GMRES, through whole RAS runs and through the C++ mirror."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hp_reference import Pattern, parilu_numpy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
MPIEXEC = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
DRIVER = os.path.join(ROOT, "schwarz-lib_amd", "build", "parilu_driver")


# ---- numpy restatements -------------------------------------------------------------------------

def _tri(rp, col, val, n):
    import scipy.sparse as sp
    return sp.csr_matrix((val, col, rp), shape=(n, n))


def neumann_numpy(f, b, k):
    """Each factor T = D + T_s applied by k Jacobi sweeps from x0 = D^-1 b."""
    n = len(f["l_rp"]) - 1
    out = b
    for name in ("l", "u"):
        T = _tri(f[name + "_rp"], f[name + "_col"], f[name + "_val"], n)
        d = T.diagonal()
        Ts = T - _diag(d)
        x = out / d
        for _ in range(k):
            x = (out - Ts @ x) / d
        out = x
    return out


def _diag(d):
    import scipy.sparse as sp
    return sp.diags(d, format="csr")


def levels(rp, col, lower):
    n = len(rp) - 1
    lv = np.zeros(n, dtype=np.int64)
    order = range(n) if lower else range(n - 1, -1, -1)
    for i in order:
        cs = col[rp[i]:rp[i + 1]]
        dep = cs[cs < i] if lower else cs[cs > i]
        lv[i] = lv[dep].max() + 1 if len(dep) else 0
    return int(lv.max()) + 1 if n else 0


# ---- cases ----------------------------------------------------------------------------------------

def _cases(oracle, convdiff):
    g = np.load(os.path.join(G, "ani4_crop.npz"))
    return {
        "lap2d_16": oracle.laplacian2d(16),
        "lap3d_12": oracle.laplacian3d(12, 12, 12),
        "convdiff_32": convdiff(32),
        "ani4_crop": (g["rp"].astype(np.int32), g["col"].astype(np.int32), g["val"]),
        "lap2d_100": oracle.laplacian2d(100),   # above 8192 rows
        "lap2d_330": oracle.laplacian2d(330),   # nnz = 543 180 > 524 288: the entry-parallel sweeps stride
    }


CASES = ["lap2d_16", "lap3d_12", "convdiff_32", "ani4_crop", "lap2d_100", "lap2d_330"]
_PAT = {}


def _case(oracle, convdiff, name):
    rp, col, val = _cases(oracle, convdiff)[name]
    rp, col, val = np.asarray(rp, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64)
    if name not in _PAT:
        _PAT[name] = Pattern(rp, col)
    return rp, col, val, _PAT[name]


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_parilu_reaches_ilu0_once_sweeps_cover_the_chains(schwz, oracle, convdiff, name):
    rp, col, val, pat = _case(oracle, convdiff, name)
    ref = schwz.ilu0(rp, col, val)
    sweeps = pat.depth()
    if name == "lap2d_16":
        sweeps = max(sweeps, len(rp) - 1)   # sweeps = n: always enough
    f = schwz.parilu(rp, col, val, sweeps)
    for k in ("l_rp", "l_col", "u_rp", "u_col"):
        assert np.array_equal(f[k], ref[k]), k
    assert _rel(f["l_val"], ref["l_val"]) <= 1e-12
    assert _rel(f["u_val"], ref["u_val"]) <= 1e-12
    # one sweep is not exact yet (the test would show nothing otherwise; the values themselves settle to
    # rounding level well before the structural chain ends)
    if pat.depth() > 2:
        g = schwz.parilu(rp, col, val, 1)
        assert max(_rel(g["l_val"], ref["l_val"]), _rel(g["u_val"], ref["u_val"])) > 1e-12


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("sweeps", [1, 2, 3])
def test_parilu_finite_sweeps_match_numpy(schwz, oracle, convdiff, name, sweeps):
    rp, col, val, pat = _case(oracle, convdiff, name)
    f = schwz.parilu(rp, col, val, sweeps)
    lv, uv = parilu_numpy(pat, val, sweeps)
    assert np.array_equal(f["l_col"], pat.l_col) and np.array_equal(f["u_col"], pat.u_col)
    assert _rel(f["l_val"], lv) <= 1e-13
    assert _rel(f["u_val"], uv) <= 1e-13


def test_parilu_zero_pivot_is_refused(schwz):
    rp = np.array([0, 2, 4], dtype=np.int32)
    col = np.array([0, 1, 0, 1], dtype=np.int32)
    val = np.array([0.0, 1.0, 1.0, 1.0])
    for sweeps in (1, 2, 5):
        with pytest.raises(schwz.SchwzError) as e:
            schwz.parilu(rp, col, val, sweeps)
        assert e.value.code == schwz.capi.ERR_NOT_SPD
        assert "%d ParILU sweep" % sweeps in str(e.value)
    with pytest.raises(schwz.SchwzError):
        schwz.parilu(np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, 1.0]), 0)


def _trs_apply(torch, t, b):
    d_b = torch.tensor(b, device="cuda", dtype=torch.float64)
    d_y = torch.full_like(d_b, float("nan"))
    t.solve(d_b.data_ptr(), d_y.data_ptr())
    torch.cuda.synchronize()
    return d_y.cpu().numpy()


@pytest.mark.parametrize("name", ["lap2d_16", "convdiff_32", "ani4_crop", "lap2d_100"])
def test_jacobi_sweep_solves(schwz, oracle, convdiff, torch_cuda, name):
    rp, col, val, _ = _case(oracle, convdiff, name)
    f = schwz.ilu0(rp, col, val)
    n = len(rp) - 1
    b = np.random.default_rng(5).standard_normal(n)
    for k in (1, 2, 3, 4):
        t = schwz.TrsSweeps(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"], k)
        assert t.sweeps == k
        for _ in range(2):
            y = _trs_apply(torch_cuda, t, b)
            assert _rel(y, neumann_numpy(f, b, k)) <= 1e-13
        t.close()
    # exact once k >= levels - 1 of both factors
    k = max(levels(f["l_rp"], f["l_col"], True), levels(f["u_rp"], f["u_col"], False)) - 1
    exact = schwz.Trs(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"])
    t = schwz.TrsSweeps(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"], k)
    y0, y1 = _trs_apply(torch_cuda, exact, b), _trs_apply(torch_cuda, t, b)
    assert _rel(y1, y0) <= 1e-12


def _solve(torch, solver, A_arrays, rtol, max_iters):
    rp, col, val = A_arrays
    n = len(rp) - 1
    d_b = torch.ones(n, device="cuda", dtype=torch.float64)
    d_x = torch.zeros(n, device="cuda", dtype=torch.float64)
    it, _ = solver.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, max_iters)
    x = d_x.cpu().numpy()
    A = _tri(rp, col, val, n)
    return it, np.linalg.norm(1.0 - A @ x) / np.sqrt(n)


def test_pcg_and_gmres_with_parilu_options(schwz, oracle, convdiff, torch_cuda):
    P = schwz.capi.PRECOND_ILU
    A = oracle.laplacian3d(32, 32, 32)
    csr = schwz.Csr(*A)
    it, rel = _solve(torch_cuda, schwz.Pcg(csr, P, par_ilu_sweeps=5, trisolve_sweeps=3), A, 1e-10, 2000)
    assert 0 < it < 2000 and rel <= 1e-9, (it, rel)
    it_exact, rel_exact = _solve(torch_cuda, schwz.Pcg(csr, P), A, 1e-10, 2000)
    # sweep counts that make both stages exact: the ParILU dependency depth, the factors' levels - 1
    f = schwz.ilu0(*A)
    par = Pattern(np.asarray(A[0]), np.asarray(A[1])).depth()
    tri = max(levels(f["l_rp"], f["l_col"], True), levels(f["u_rp"], f["u_col"], False)) - 1
    it_big, rel_big = _solve(torch_cuda, schwz.Pcg(csr, P, par_ilu_sweeps=par, trisolve_sweeps=tri), A, 1e-10, 2000)
    assert it_big == it_exact, (it_big, it_exact)
    assert abs(rel_big - rel_exact) <= 1e-3 * rel_exact + 1e-15
    C = convdiff(64)
    it_g, rel_g = _solve(torch_cuda, schwz.Gmres(schwz.Csr(*C), P, restart=30, par_ilu_sweeps=5, trisolve_sweeps=3),
                         C, 1e-10, 3000)
    assert 0 < it_g < 3000 and rel_g <= 1e-8, (it_g, rel_g)
    # the refusals of schwz_pcg_create_ilu / schwz_gmres_create_ex
    with pytest.raises(schwz.NotImplementedSchwz):
        schwz.Pcg(csr, schwz.capi.PRECOND_ISAI, trisolve_sweeps=2)
    with pytest.raises(schwz.NotImplementedSchwz):
        schwz.Gmres(csr, schwz.capi.PRECOND_JACOBI, restart=10, par_ilu_sweeps=2)
    with pytest.raises(schwz.SchwzError) as e:
        schwz.Pcg(csr, P, par_ilu_sweeps=-1)
    assert e.value.code == schwz.capi.ERR_INVALID


# ---- whole RAS runs -----------------------------------------------------------------------------

def _run(schwz, P, settings_kw, metadata_kw):
    s = schwz.Settings(**settings_kw)
    m = schwz.Metadata(num_subdomains=P, **metadata_kw)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    return solver, m, solver.run()


def _lambda_min(shape):
    return sum(4.0 * np.sin(np.pi / (2 * (k + 1))) ** 2 for k in shape)


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("opts", [("ilu", 5, 3), ("ilu", 0, 2), ("ilu", 3, 0), ("isai", 5, 0)])
def test_ras_with_parilu_options(schwz, oracle, torch_cuda, P, opts):
    name, par, tri = opts
    for dims, tol in (((30, 30), 1e-8), ((22, 21, 40), 1e-7)):
        sk = dict() if len(dims) == 2 else dict(laplacian_dim=3, laplacian_shape=dims)
        mk = dict(oned_laplacian_size=dims[0]) if len(dims) == 2 else dict()
        solver, m, out = _run(schwz, P, sk, dict(mk, tolerance=tol, max_iters=400, local_precond=name,
                                                 local_solver_tolerance=1e-10, par_ilu_sweeps=par,
                                                 trisolve_sweeps=tri))
        assert out["converged"], (dims, out["iter_count"])
        A = oracle.laplacian2d(dims[0]) if len(dims) == 2 else oracle.laplacian3d(*dims)
        N = len(A[0]) - 1
        fr = np.asarray(m.first_row, dtype=np.int32)
        r = oracle.ras_run(*A, np.ones(N), P, fr,
                           oracle.make_settings(max_iters=400, tol=tol, precond=oracle.precond_code(name)[0],
                                                local_tol=1e-10))
        assert r["converged"]
        x = np.asarray(out["solution"])
        res = np.linalg.norm(np.ones(N) - _tri(*A, N) @ x)
        # the outer test is on the subdomain residuals relative to the first ones (x0 = 0: the rhs norm); the
        # assembled solution's true residual meets the tolerance within the slack of that criterion
        assert res <= 10 * tol * np.sqrt(N), (res, tol)
        # both runs meet the tolerance: |x - x_oracle| <= (|r| + |r_oracle|) / lambda_min
        res_o = np.linalg.norm(np.ones(N) - _tri(*A, N) @ r["solution"])
        assert np.linalg.norm(x - r["solution"]) <= (res + res_o) / _lambda_min(dims)


@pytest.mark.parametrize("P", [1, 3])
def test_ras_exact_sweep_counts_reproduce_the_exact_ilu_run(schwz, oracle, torch_cuda, P):
    n = 30
    base = dict(oned_laplacian_size=n, tolerance=1e-8, max_iters=300, local_precond="ilu",
                local_solver_tolerance=1e-10)
    solver, m, out0 = _run(schwz, P, dict(), base)
    par = tri = 1
    for sd in solver.subdomains.values():
        rp, col, val = sd.local_matrix()
        par = max(par, Pattern(rp, col).depth())
        f = schwz.ilu0(rp, col, val)
        tri = max(tri, levels(f["l_rp"], f["l_col"], True) - 1, levels(f["u_rp"], f["u_col"], False) - 1)
    _, _, out1 = _run(schwz, P, dict(), dict(base, par_ilu_sweeps=par, trisolve_sweeps=tri))
    assert out1["converged"] and out0["converged"]
    assert out1["iter_count"] == out0["iter_count"]
    scale = np.abs(out0["solution"]).max()
    assert np.abs(np.asarray(out1["solution"]) - out0["solution"]).max() <= 1e-8 * scale


def test_zero_sweep_fields_change_nothing(schwz, torch_cuda):
    shape = (22, 21, 40)
    kw = dict(tolerance=1e-7, max_iters=300, local_precond="ilu", local_solver_tolerance=1e-10)
    s_kw = dict(laplacian_dim=3, laplacian_shape=shape)
    s0, _, out0 = _run(schwz, 2, s_kw, kw)
    s1, _, out1 = _run(schwz, 2, s_kw, dict(kw, par_ilu_sweeps=0, trisolve_sweeps=0))
    assert out0["iter_count"] == out1["iter_count"]
    assert np.array_equal(np.asarray(out0["solution"]), np.asarray(out1["solution"]))
    assert out0["residual_norm"] == out1["residual_norm"]
    for me in s0.subdomains:
        assert s0.subdomains[me].cg_flavour() == s1.subdomains[me].cg_flavour()


# ---- C++ mirror -----------------------------------------------------------------------------------

def _driver(nranks, *args):
    if not os.path.exists(DRIVER):
        pytest.skip("parilu_driver not built (`make -C schwarz-lib_amd parilu_driver`, needs MPI)")
    if not os.path.exists(MPIEXEC):
        pytest.skip("no mpiexec on this machine")
    cmd = [MPIEXEC, "-n", str(nranks), DRIVER] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("args", [("ilu", 5, 3), ("isai", 5, 0)])
def test_mirror_parilu_options_converge(oracle, args):
    name, par, tri = args
    p = _driver(2, name, 32, par, tri, 1e-8, 300)
    assert p.returncode == 0, p.stdout + p.stderr
    res = re.search(r"RESULT iters=(\d+) solnorm=([0-9.eE+-]+)", p.stdout)
    assert res, p.stdout
    assert 0 < int(res.group(1)) < 300
    rp, col, val = oracle.laplacian2d(32)
    x = _spsolve(rp, col, val)
    assert abs(float(res.group(2)) - np.linalg.norm(x)) <= 1e-6 * np.linalg.norm(x)


def test_mirror_refuses_trisolve_sweeps_with_isai():
    p = _driver(1, "isai", 32, 5, 2, 1e-8, 300)
    assert p.returncode == 3, p.stdout + p.stderr
    assert "REFUSED" in p.stdout


def _spsolve(rp, col, val):
    import scipy.sparse.linalg as sl
    n = len(rp) - 1
    return sl.spsolve(_tri(rp, col, val, n).tocsc(), np.ones(n))
