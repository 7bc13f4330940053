"""SolverRAS.run() with outer_iteration = "fgmres" (schwz_amd/outer.py) on the 32 x 32 x 8 seven-point Laplacian
(8192 rows, handed over through initialize(matrix=...)), eight in-process subdomains, regular partition, overlap 2, a
random right-hand side with a fixed seed, tolerance 1e-8.

The reference is a float64 FGMRES written here, whose preconditioner is assembled from the project's own index sets and
local matrices (local_to_global, local_size, local_matrix()): M^-1 v = sum_i R~_i^T A_i^-1 R_i v.  It runs in four
variants -- modified Gram-Schmidt and classical Gram-Schmidt applied twice, each with SuperLU and with dense local
solves -- whose largest mutual relative difference in history[k] / history[0] is the SPREAD: what float64 arithmetic
leaves undetermined in these numbers.  The device has to agree with the reference within 1000 x spread + 1e-13 wherever
the reference ratio is >= 1e-6.  The figures are printed, and appended to the file SCHWZ_OUTER_PARITY_LOG names.

The non-symmetric case adds a first-order upwind convection term; its direct local solver is the pivoted LU
(local_solver "direct-ginkgo" with factorization "umfpack": this project's spelling of the reference's
direct-umfpack)."""
import os

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu
SHAPE = (32, 32, 8)
N = 32 * 32 * 8
P = 8
TOL = 1e-8
CHOLMOD = dict(local_solver="direct-cholmod")
UMFPACK = dict(local_solver="direct-ginkgo", factorization="umfpack", non_symmetric_matrix=True)
JACOBI_CG10 = dict(local_precond="block-jacobi", precond_max_block_size=1, local_solver_tolerance=0.0, local_max_iters=10)


def matrix(kind):
    nx, ny, nz = SHAPE

    def lap1(n):
        return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n), format="csr")

    def up1(n):
        return sp.diags([-1.0, 1.0], [-1, 0], shape=(n, n), format="csr")
    ex, ey, ez = (sp.identity(n, format="csr") for n in (nx, ny, nz))
    a = sp.kron(ez, sp.kron(ey, lap1(nx))) + sp.kron(ez, sp.kron(lap1(ny), ex)) + sp.kron(lap1(nz), sp.kron(ey, ex))
    if kind == "convection":
        a = a + 1.5 * sp.kron(ez, sp.kron(ey, up1(nx))) - 0.75 * sp.kron(ez, sp.kron(up1(ny).T, ex)) \
            + 0.5 * sp.kron(up1(nz), sp.kron(ey, ex))
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    return a


def rhs():
    return np.random.default_rng(20260127).standard_normal(N)


_cache = {}


def make_solver(schwz, kind, settings, outer="fgmres", restart=30, max_iters=200, tol=TOL, **metadata):
    a = matrix(kind)
    s = schwz.Settings(**settings)
    m = schwz.Metadata(num_subdomains=P, tolerance=tol, max_iters=max_iters, outer_iteration=outer,
                       outer_restart=restart, **metadata)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize(matrix=(a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float64)),
                      rhs=rhs())
    assert m.permutation is None and s.overlap == 2 and len(solver.subdomains) == P
    return solver


def device_run(schwz, kind, settings, restart=30, **metadata):
    """(solver, result) of an FGMRES run: computed once per configuration, never written to."""
    key = (kind, tuple(sorted(settings.items())), restart, tuple(sorted(metadata.items())))
    if key not in _cache:
        solver = make_solver(schwz, kind, settings, restart=restart, **metadata)
        _cache[key] = (solver, solver.run())
    return _cache[key]


# ---- the reference ------------------------------------------------------------------------------------------------------

def preconditioner(solver, dense):
    """M^-1 from the solver's own subdomains: exact local solves on [interior | overlap], the interior kept."""
    parts = []
    for me in sorted(solver.subdomains):
        sd = solver.subdomains[me]
        nx = sd.local_size_x
        rp, col, val = sd.local_matrix()
        a = sp.csr_matrix((val, col, rp), shape=(nx, nx))
        # (dense: LAPACK's LU of the full matrix, factored once -- numpy.linalg.solve, which factors again at every
        # application of a matrix of up to 3072 rows, is the same getrf / getrs pair)
        solve = (lambda v, f=scipy.linalg.lu_factor(a.toarray()): scipy.linalg.lu_solve(f, v)) if dense \
            else spla.splu(a.tocsc()).solve
        parts.append((np.asarray(sd.local_to_global[:nx], dtype=np.int64), int(sd.local_size), solve))

    def apply(v):
        z = np.zeros_like(v)
        for l2g, n, solve in parts:
            z[l2g[:n]] = solve(v[l2g])[:n]
        return z
    return apply


def fgmres(a, b, minv, restart, tol, max_iters, cgs2):
    """Right-preconditioned flexible GMRES(restart) from a zero start; history[k] after k applications: the recomputed
    residual at k = 0, afterwards the residual of the small least-squares problem (numpy.linalg.lstsq)."""
    n = len(b)
    x = np.zeros(n)
    bnorm = np.linalg.norm(b)
    r = b - a @ x
    beta = np.linalg.norm(r)
    history, apps = [beta], 0
    while history[-1] > tol * bnorm and apps < max_iters:
        V, Z, H = np.zeros((restart + 1, n)), np.zeros((restart, n)), np.zeros((restart + 1, restart))
        V[0] = r / beta
        k = 0
        for j in range(restart):
            Z[j] = minv(V[j])
            w = a @ Z[j]
            if cgs2:
                h1 = V[:j + 1] @ w
                w = w - V[:j + 1].T @ h1
                h2 = V[:j + 1] @ w
                w = w - V[:j + 1].T @ h2
                H[:j + 1, j] = h1 + h2
            else:
                for i in range(j + 1):
                    H[i, j] = V[i] @ w
                    w = w - H[i, j] * V[i]
            H[j + 1, j] = np.linalg.norm(w)
            V[j + 1] = w / H[j + 1, j]
            k, apps = j + 1, apps + 1
            e1 = np.zeros(k + 1)
            e1[0] = beta
            y = np.linalg.lstsq(H[:k + 1, :k], e1, rcond=None)[0]
            history.append(np.linalg.norm(e1 - H[:k + 1, :k] @ y))
            if history[-1] <= tol * bnorm or apps >= max_iters:
                break
        x = x + Z[:k].T @ y
        r = b - a @ x
        beta = np.linalg.norm(r)
    return np.array(history), apps, x


def references(schwz, kind, settings):
    """The four variants on the index sets of the device solver; (histories, spread, the CGS2 / SuperLU run)."""
    key = ("ref", kind)
    if key not in _cache:
        solver, _ = device_run(schwz, kind, settings)
        a, b = matrix(kind), rhs()
        runs = [fgmres(a, b, minv, 30, TOL, 200, cgs2)
                for minv in (preconditioner(solver, False), preconditioner(solver, True)) for cgs2 in (True, False)]
        ratios = [h / h[0] for h, _, _ in runs]
        kmax = min(len(r) for r in ratios)
        keep = ratios[0][:kmax] >= 1e-6
        spread = max(float(np.max(np.abs(ra[:kmax][keep] - rb[:kmax][keep]) / ratios[0][:kmax][keep]))
                     for ra in ratios for rb in ratios)
        _cache[key] = (ratios, spread, runs[0])
    return _cache[key]


def parity(schwz, kind, settings):
    _, out = device_run(schwz, kind, settings)
    ratios, spread, (ref_hist, ref_apps, ref_x) = references(schwz, kind, settings)
    ref = ratios[0]
    dev = np.array(out["history"]) / out["history"][0]
    kmax = min(len(ref), len(dev))
    keep = ref[:kmax] >= 1e-6
    diff = float(np.max(np.abs(dev[:kmax][keep] - ref[:kmax][keep]) / ref[:kmax][keep]))
    line = ("outer FGMRES parity, %s: spread of the four float64 references %.3e, device against CGS2/SuperLU %.3e "
            "(bound %.3e), applications device %d / reference %d" %
            (kind, spread, diff, 1000 * spread + 1e-13, out["iter_count"], ref_apps))
    print(line)
    if os.environ.get("SCHWZ_OUTER_PARITY_LOG"):
        with open(os.environ["SCHWZ_OUTER_PARITY_LOG"], "a") as f:
            f.write(line + "\n")
    assert out["converged"]
    assert keep.sum() >= 5
    assert diff <= 1000 * spread + 1e-13
    assert abs(out["iter_count"] - ref_apps) <= 1
    assert len(out["history"]) == out["iter_count"] + 1
    assert out["history"][-1] <= TOL * np.linalg.norm(rhs())


# ---- the tests --------------------------------------------------------------------------------------------------------

def test_linear_parity_cholmod(schwz):
    parity(schwz, "laplacian", CHOLMOD)


def test_linear_parity_nonsymmetric_lu(schwz):
    parity(schwz, "convection", UMFPACK)


def test_result_is_the_solution(schwz):
    """The tail of run() applies: the solution, its true residual and the norms, against the host."""
    _, out = device_run(schwz, "laplacian", CHOLMOD)
    a, b = matrix("laplacian"), rhs()
    true = np.linalg.norm(b - a @ out["solution"])
    assert out["rhs_norm"] == pytest.approx(np.linalg.norm(b), rel=1e-14)
    assert out["residual_norm"] == pytest.approx(true, rel=1e-6)
    assert true <= 1.01 * TOL * np.linalg.norm(b)
    assert set(out) >= {"iter_count", "converged", "elapsed", "residual_norm", "rhs_norm", "sol_norm", "solution", "history"}
    assert out["cycle_starts"][0] == (0, out["history"][0])


def richardson_true_residuals(schwz, upto):
    """What a stationary run() capped at max_iters = k returns as residual_norm, for k = 1 .. upto, from ONE pass
    over the iteration (a direct local solve of these 3072-row subdomains costs a third of a second per outer
    iteration, so upto separate runs would take minutes): begin_run(), then step() by step() what the tail of run()
    does after its last step -- the exchange and the sum of schwz_ras_true_residual_sq.  The exchange rewrites halo
    slots with the values the next step's own exchange writes again, so the iteration is not disturbed.  A tolerance
    of 0 never fires.  Checked against a real capped run at k = 1."""
    key = ("richardson", upto)
    if key not in _cache:
        solver = make_solver(schwz, "laplacian", CHOLMOD, outer="richardson", tol=0.0, max_iters=upto)
        stream = solver.backend.stream()
        solver.begin_run()
        res = {}
        for k in range(1, upto + 1):
            assert solver.step() is False
            solver._exchange()
            res[k] = float(np.sqrt(sum(sd.true_residual_sq(stream) for sd in solver.subdomains.values())))
        solver.metadata.max_iters = 1
        capped = solver.solve(rhs(), "zero", gather_solution=False)
        assert capped["iter_count"] == 1 and capped["residual_norm"] == pytest.approx(res[1], rel=1e-13)
        _cache[key] = res
    return _cache[key]


def test_never_worse_than_richardson(schwz):
    """Exact-arithmetic GMRES minimises the residual over a space that contains the stationary iterate."""
    _, out = device_run(schwz, "laplacian", CHOLMOD)
    kf = out["iter_count"]
    assert kf >= 10
    rich = richardson_true_residuals(schwz, kf)
    for k in (1, 5, 10):
        assert out["history"][k] <= (1.0 + 1e-8) * rich[k], (k, out["history"][k], rich[k])
    # ... and fewer applications to the same true residual: the stationary iteration has not reached it after kf
    assert all(rich[k] > out["residual_norm"] for k in range(1, kf + 1)), (out["residual_norm"], rich)


def test_flexible_with_ten_cg_iterations(schwz):
    """Jacobi-CG with local_max_iters = 10 and no local tolerance is not a fixed linear operator.  The run converges,
    and the true residual of the returned solution, recomputed on the host, is the last history entry to within a
    tenth of the tolerance: a condition that makes the stop test trustworthy to 10 %, not a measurement."""
    _, out = device_run(schwz, "laplacian", {}, **JACOBI_CG10)
    a, b = matrix("laplacian"), rhs()
    assert out["converged"] and out["iter_count"] < 200
    true = np.linalg.norm(b - a @ out["solution"])
    assert abs(true - out["history"][-1]) <= 0.1 * TOL * np.linalg.norm(b), (true, out["history"][-1])


def test_restart_five(schwz):
    _, long_ = device_run(schwz, "laplacian", CHOLMOD)
    _, short = device_run(schwz, "laplacian", CHOLMOD, restart=5)
    assert short["converged"] and len(short["cycle_starts"]) > 1 and short["iter_count"] > 5
    assert [k for k, _ in short["cycle_starts"][:2]] == [0, 5]
    assert np.array(short["history"][:6]).tobytes() == np.array(long_["history"][:6]).tobytes()
    # the recomputed residual that starts the second cycle is the recurrence's, to rounding
    assert short["cycle_starts"][1][1] == pytest.approx(short["history"][5], rel=1e-8)


def test_state_hygiene(schwz):
    """After an FGMRES solve the solver is an ordinary one again: with outer_iteration = "richardson",
    solve(b, "zero") is bit for bit a fresh solver's run, and "keep" after FGMRES starts from its solution."""
    # (every run is capped at a few outer iterations: what is compared are bits, not converged solutions, and a direct
    # local solve of these subdomains costs a third of a second per outer iteration)
    b = rhs()
    solver = make_solver(schwz, "laplacian", CHOLMOD, max_iters=7)
    sol = solver.run()
    assert sol["iter_count"] == 7 and not sol["converged"] and len(sol["history"]) == 8
    assert sol["residual_norm"] == pytest.approx(sol["history"][-1], rel=1e-8)
    # "keep" after FGMRES starts from its solution: FGMRES finds the residual it ended with ...
    solver.metadata.max_iters = 0
    kept = solver.solve(b, "keep")
    assert kept["iter_count"] == 0 and len(kept["history"]) == 1
    assert kept["history"][0] == pytest.approx(sol["residual_norm"], rel=1e-10)
    assert kept["solution"].tobytes() == sol["solution"].tobytes()
    # ... and so does the tail of the stationary loop
    solver.metadata.outer_iteration = "richardson"
    rich = solver.solve(b, "keep")
    assert rich["iter_count"] == 0 and rich["residual_norm"] == pytest.approx(sol["residual_norm"], rel=1e-10)
    assert rich["solution"].tobytes() == sol["solution"].tobytes()
    # "zero": bit for bit a fresh solver's run -- counts, residual histories, solution
    solver.metadata.max_iters = 6
    again = solver.solve(b, "zero")
    fresh = make_solver(schwz, "laplacian", CHOLMOD, outer="richardson", max_iters=6)
    ref = fresh.run()
    assert again["iter_count"] == ref["iter_count"] == 6 and again["converged"] == ref["converged"]
    assert again["solution"].tobytes() == ref["solution"].tobytes()
    assert again["residual_norm"] == ref["residual_norm"]
    ppd_a, ppd_r = solver.metadata.post_process_data, fresh.metadata.post_process_data
    assert len(ppd_r["local_residual_vector_out"]) == 6 * P
    assert ppd_a["local_residual_vector_out"] == ppd_r["local_residual_vector_out"]
    assert ppd_a["global_residual_vector_out"] == ppd_r["global_residual_vector_out"]


def test_one_subdomain(schwz, oracle):
    """No overlap rows, no halo: the operator pass writes w itself and y may be the x~ buffer.  With local solves to
    1e-12 the preconditioner is nearly A^-1: a handful of applications, and the solution is the host's."""
    shape = (16, 10, 7)
    n = shape[0] * shape[1] * shape[2]
    rp, col, val = oracle.laplacian3d(*shape)
    a = sp.csr_matrix((val, col, rp), shape=(n, n))
    b = np.random.default_rng(3).standard_normal(n)
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=shape)
    m = schwz.Metadata(num_subdomains=1, tolerance=1e-10, max_iters=20, outer_iteration="fgmres", outer_restart=4,
                       local_precond="block-jacobi", precond_max_block_size=1, local_solver_tolerance=1e-12)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(1), quiet=True)
    solver.initialize(rhs=b)
    out = solver.run()
    assert out["converged"] and 1 <= out["iter_count"] <= 4
    true = np.linalg.norm(b - a @ out["solution"])
    assert abs(true - out["history"][-1]) <= 0.1 * 1e-10 * np.linalg.norm(b)
    x = spla.spsolve(a.tocsc(), b)
    assert np.abs(out["solution"] - x).max() <= 1e-8 * np.abs(x).max()


def test_a_nan_is_diverged(schwz):
    solver = make_solver(schwz, "laplacian", CHOLMOD)
    bad = rhs()
    solver.set_rhs(bad, "zero")
    import torch
    for sd in solver.subdomains.values():  # (set_rhs refuses a NaN: it is written behind its back)
        p, n = sd.vector(3)
        nan = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        schwz.outer_copy(1, nan.data_ptr(), p)
        break
    with pytest.raises(schwz.SchwzError) as e:
        solver.run()
    assert e.value.code == schwz.capi.ERR_DIVERGED
