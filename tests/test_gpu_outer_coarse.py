"""SolverRAS.run() with outer_iteration = "fgmres" and outer_preconditioner = "two-level" (schwz_amd/outer.py) on the
problem of test_gpu_outer_ras.py: the 32 x 32 x 8 seven-point Laplacian and its convection variant, eight in-process
subdomains (one z-plane each), overlap 2, the same seeded right-hand side, tolerance 1e-8, max_iters 200.  The coarse
space: 8 x 8 x 1 boxes per plane, aggregate id 16 z + 4 (y // 8) + x // 8, nc = 128.

The reference is the float64 FGMRES of that file with the preconditioner assembled on the host from the solver's own
index sets, local matrices and aggregate ids,

    M^-1 v = z0 + RAS(v - A z0),   z0 = Z (Z^T A Z)^-1 Z^T v,

in the same four variants (SuperLU or dense local solves, each with CGS2 and with MGS), whose mutual difference is the
SPREAD.  The device has to agree with the CGS2 / SuperLU run within that file's rule, 1000 x spread + 1e-13 wherever the
reference ratio is >= 1e-6, on at least five such entries."""
import os

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import test_gpu_outer_ras as one_level
from test_gpu_outer_ras import CHOLMOD, JACOBI_CG10, N, P, SHAPE, TOL, UMFPACK, fgmres, make_solver, matrix, preconditioner, rhs
from test_gpu_coarse import boxes

pytestmark = pytest.mark.gpu
NC = 128


def aggregates():
    nx, ny, nz = SHAPE
    i = np.arange(N)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    return (16 * z + 4 * (y // 8) + x // 8).astype(np.int64)


def two_level(**metadata):
    return dict(coarse_space="aggregates", coarse_aggregate_vector=aggregates(), outer_preconditioner="two-level", **metadata)


_cache = {}


def device_run(schwz, kind, settings, restart=30, **metadata):
    """(solver, result) of a two-level FGMRES run: computed once per configuration, never written to."""
    key = (kind, tuple(sorted(settings.items())), restart, tuple(sorted(metadata.items())))
    if key not in _cache:
        solver = make_solver(schwz, kind, settings, restart=restart, **two_level(**metadata))
        assert solver._coarse["nc"] == NC
        _cache[key] = (solver, solver.run())
    return _cache[key]


def two_level_preconditioner(solver, a, dense):
    """M^-1 of the module docstring from the solver's own subdomains and aggregate ids."""
    ras = preconditioner(solver, dense)
    ids = np.empty(N, dtype=np.int64)
    for me, sd in solver.subdomains.items():
        ids[np.asarray(sd.local_to_global[:sd.local_size], dtype=np.int64)] = solver._coarse["interior"][me]
    z = sp.csr_matrix((np.ones(N), (np.arange(N), ids)), shape=(N, NC))
    a0 = scipy.linalg.lu_factor((z.T @ a @ z).toarray())

    def apply(v):
        z0 = z @ scipy.linalg.lu_solve(a0, z.T @ v)
        return z0 + ras(v - a @ z0)
    return apply


def references(schwz, kind, settings):
    """The four variants on the index sets of the device solver; (ratios, spread, the CGS2 / SuperLU run)."""
    key = ("ref", kind)
    if key not in _cache:
        solver, _ = device_run(schwz, kind, settings)
        a, b = matrix(kind), rhs()
        runs = [fgmres(a, b, minv, 30, TOL, 200, cgs2)
                for minv in (two_level_preconditioner(solver, a, False), two_level_preconditioner(solver, a, True))
                for cgs2 in (True, False)]
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
    line = ("two-level outer FGMRES parity, %s: %d entries >= 1e-6, spread of the four float64 references %.3e, device "
            "against CGS2/SuperLU %.3e (bound %.3e), applications device %d / reference %d" %
            (kind, int(keep.sum()), spread, diff, 1000 * spread + 1e-13, out["iter_count"], ref_apps))
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


@pytest.mark.parametrize("kind,settings", [("laplacian", CHOLMOD), ("convection", UMFPACK)], ids=["laplacian", "convection"])
def test_fewer_applications_than_one_level(schwz, kind, settings):
    """On the host references first, then on the device (the one-level runs are those of test_gpu_outer_ras.py)."""
    _, _, (_, ref_two, _) = references(schwz, kind, settings)
    _, _, (_, ref_one, _) = one_level.references(schwz, kind, settings)
    _, dev_two = device_run(schwz, kind, settings)
    _, dev_one = one_level.device_run(schwz, kind, settings)
    print("applications, %s: two-level device %d / reference %d, one-level device %d / reference %d"
          % (kind, dev_two["iter_count"], ref_two, dev_one["iter_count"], ref_one))
    assert ref_two < ref_one
    assert dev_two["converged"] and dev_one["converged"]
    assert dev_two["iter_count"] <= dev_one["iter_count"]


def test_flexible_with_ten_cg_iterations(schwz):
    """Jacobi-CG with local_max_iters = 10 and no local tolerance is not a fixed linear operator: no parity.  The run
    converges, history is finite and ends below the tolerance, and the true residual of the returned solution,
    recomputed on the host, is the last history entry to within a tenth of the tolerance."""
    _, out = device_run(schwz, "laplacian", {}, **JACOBI_CG10)
    a, b = matrix("laplacian"), rhs()
    assert out["converged"] and out["iter_count"] < 200
    assert np.isfinite(out["history"]).all() and out["history"][-1] <= TOL * np.linalg.norm(b)
    true = np.linalg.norm(b - a @ out["solution"])
    assert abs(true - out["history"][-1]) <= 0.1 * TOL * np.linalg.norm(b), (true, out["history"][-1])


def test_restart_five(schwz):
    _, long_ = device_run(schwz, "laplacian", CHOLMOD)
    _, short = device_run(schwz, "laplacian", CHOLMOD, restart=5)
    assert short["converged"] and len(short["cycle_starts"]) > 1 and short["iter_count"] > 5
    assert [k for k, _ in short["cycle_starts"][:2]] == [0, 5]
    assert np.array(short["history"][:6]).tobytes() == np.array(long_["history"][:6]).tobytes()
    # the recomputed residuals that start the cycles are the recurrence's, to rounding
    for k, true in short["cycle_starts"][1:]:
        assert true == pytest.approx(short["history"][k], rel=1e-8), k


def test_state_hygiene(schwz):
    """After a two-level FGMRES run the solver is an ordinary two-level one again: with outer_iteration =
    "richardson", solve(b, "zero") is bit for bit a fresh two-level solver's run() -- residual histories and solution.
    This is what fails if beta of the coarse plan, y or the solver objects' memory were left dirty."""
    b = rhs()
    solver = make_solver(schwz, "laplacian", CHOLMOD, max_iters=4, **two_level())
    sol = solver.run()
    assert sol["iter_count"] == 4 and not sol["converged"] and len(sol["history"]) == 5
    assert sol["residual_norm"] == pytest.approx(sol["history"][-1], rel=1e-8)
    solver.metadata.outer_iteration = "richardson"
    solver.metadata.max_iters = 5
    again = solver.solve(b, "zero")
    fresh = make_solver(schwz, "laplacian", CHOLMOD, outer="richardson", max_iters=5, **two_level())
    ref = fresh.run()
    assert again["iter_count"] == ref["iter_count"] == 5 and again["converged"] == ref["converged"]
    assert again["solution"].tobytes() == ref["solution"].tobytes()
    assert again["residual_norm"] == ref["residual_norm"]
    ppd_a, ppd_r = solver.metadata.post_process_data, fresh.metadata.post_process_data
    assert len(ppd_r["local_residual_vector_out"]) == 5 * P
    assert ppd_a["local_residual_vector_out"] == ppd_r["local_residual_vector_out"]
    assert ppd_a["global_residual_vector_out"] == ppd_r["global_residual_vector_out"]


def test_one_subdomain(schwz, oracle):
    """P = 1: no overlap rows, no halo, y may be the x~ buffer (the coarse apply then adds once).  With local solves to
    1e-12 the sweep alone is nearly A^-1: a handful of applications, and the solution is the host's."""
    shape = (16, 10, 7)
    n = shape[0] * shape[1] * shape[2]
    rp, col, val = oracle.laplacian3d(*shape)
    a = sp.csr_matrix((val, col, rp), shape=(n, n))
    b = np.random.default_rng(3).standard_normal(n)
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=shape)
    m = schwz.Metadata(num_subdomains=1, tolerance=1e-10, max_iters=20, outer_iteration="fgmres", outer_restart=4,
                       local_precond="block-jacobi", precond_max_block_size=1, local_solver_tolerance=1e-12,
                       coarse_space="aggregates", coarse_aggregate_vector=boxes(shape, (4, 5, 4)),
                       outer_preconditioner="two-level")
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(1), quiet=True)
    solver.initialize(rhs=b)
    assert solver._coarse["nc"] == 16
    out = solver.run()
    assert out["converged"] and 1 <= out["iter_count"] <= 4
    true = np.linalg.norm(b - a @ out["solution"])
    assert abs(true - out["history"][-1]) <= 0.1 * 1e-10 * np.linalg.norm(b)
    x = spla.spsolve(a.tocsc(), b)
    assert np.abs(out["solution"] - x).max() <= 1e-8 * np.abs(x).max()


def test_the_default_preconditioner_still_refuses(schwz):
    with pytest.raises(schwz.NotImplementedSchwz) as e:
        make_solver(schwz, "laplacian", CHOLMOD, coarse_space="aggregates", coarse_aggregate_vector=aggregates())
    assert e.value.code == schwz.capi.ERR_NOT_IMPLEMENTED and "fgmres" in str(e.value) and "outer_preconditioner" in str(e.value)


def test_profile_has_a_coarse_entry(schwz):
    solver = make_solver(schwz, "laplacian", {}, max_iters=3, **two_level(**JACOBI_CG10))
    solver.outer_profile = True
    out = solver.run()
    assert set(out["profile"]) == {"sweep", "coarse", "apply", "ortho"} and all(v > 0 for v in out["profile"].values())
