"""SolverRAS.run() with outer_iteration = "fgmres" and outer_basis = "single" (schwz_amd/outer.py: the Krylov basis V in
fp32, everything else fp64) on the problems of test_gpu_outer_ras.py: the 32 x 32 x 8 Laplacian and its convection
variant on eight in-process subdomains, the same seeded right-hand side.

The reference is a float64 host FGMRES with M^-1 assembled from the solver's own index sets and local matrices (the
helpers of test_gpu_outer_ras.py and test_gpu_outer_coarse.py), which rounds V to fp32 at the same two places (v_0 and
every v_(j+1)) and recomputes b - A x at the same places (every cycle end), in four variants: CGS2 or MGS, crossed with
SuperLU or dense LU.  A cycle that starts from a residual at the rounding floor is a different trajectory in each
variant, so histories are compared only where that is meaningful: over the first cycle at restart 30, over all cycles
at restart 5.  The measure is |device - CGS2/SuperLU reference| / (start residual of the entry's cycle), the margin
10 x the largest pairwise value among the four host variants: the device differs from them in the ways they differ
from one another (summation order, fused multiply-adds, which entries round the other way).

The test that matters is the truth of the answer: `converged` is said of a recomputed residual only, and ||b - A x||
evaluated in np.longdouble from the RETURNED solution agrees with history[-1] within the rounding bound of evaluating
that residual, (max row length + 2) 2^-52 || |b| + |A||x| ||_2.

Figures the tests print (and append to the file SCHWZ_OUTER_PARITY_LOG names): the spread and the device's deviation
per parity case; the application counts of device / host variants / double-basis device.  Measured on the MI355X
(profiles/r29_outer_basis.txt): spread / device 6.0e-11 / 4.9e-17 (cholmod), 3.4e-11 / 7.1e-18 (pivoted LU, convection),
2.8e-11 / 7.9e-17 (two-level) over the first cycle at restart 30, 5.6e-8 / 1.1e-8 over all cycles at restart 5;
applications single / double 22 / 21 and 17 / 16 (two-level) at 1e-8, 42 / 30 and 31 / 23 at 1e-12.

The direct local solves of these 3072-row subdomains cost a third of a second per application, so the runs are shared
between the tests of this file and the longest test (1e-12, with its double-basis counterpart) takes about 28 s."""
import os

import numpy as np
import pytest

import test_gpu_outer_coarse as coarse
from test_gpu_outer_ras import CHOLMOD, JACOBI_CG10, N, P, UMFPACK, make_solver, matrix, preconditioner, rhs

pytestmark = pytest.mark.gpu
LD = np.longdouble
_cache = {}


def log(line):
    print(line)
    if os.environ.get("SCHWZ_OUTER_PARITY_LOG"):
        with open(os.environ["SCHWZ_OUTER_PARITY_LOG"], "a") as f:
            f.write(line + "\n")


def device_run(schwz, kind, settings, basis="single", restart=30, tol=1e-8, two=False, max_iters=200, **metadata):
    """(solver, result): computed once per configuration, never written to."""
    key = (kind, tuple(sorted(settings.items())), basis, restart, tol, two, max_iters, tuple(sorted(metadata.items())))
    if key not in _cache:
        md = dict(metadata)
        if basis is not None:
            md["outer_basis"] = basis
        if two:
            md = coarse.two_level(**md)
        solver = make_solver(schwz, kind, settings, restart=restart, tol=tol, max_iters=max_iters, **md)
        _cache[key] = (solver, solver.run())
    return _cache[key]


# ---- the reference ------------------------------------------------------------------------------------------------------

def fl32(v):
    return v.astype(np.float32).astype(np.float64)


def fgmres_single(a, b, minv, restart, tol, max_iters, cgs2):
    """test_gpu_outer_ras.fgmres with the basis vectors rounded to fp32 where they are stored and b - A x recomputed at
    every cycle end, its norm the last entry of the cycle; another cycle where that misses the tolerance.
    (history, applications, x, cycle_starts)."""
    n = len(b)
    x = np.zeros(n)
    bnorm = np.linalg.norm(b)
    r = b - a @ x
    beta = np.linalg.norm(r)
    history, apps, starts = [beta], 0, [(0, beta)]
    while history[-1] > tol * bnorm and apps < max_iters:
        V, Z, H = np.zeros((restart + 1, n)), np.zeros((restart, n)), np.zeros((restart + 1, restart))
        V[0] = fl32(r / beta)
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
            V[j + 1] = fl32(w / H[j + 1, j])
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
        history[-1] = beta
        starts.append((apps, beta))
    return np.array(history), apps, x, starts


def references(schwz, kind, settings, restart, tol, two):
    """The four variants on the index sets of the device solver: [(history, applications, x, cycle_starts)], CGS2 /
    SuperLU first."""
    key = ("ref", kind, restart, tol, two)
    if key not in _cache:
        solver, _ = device_run(schwz, kind, settings, restart=restart, tol=tol, two=two)
        a, b = matrix(kind), rhs()
        make = (lambda dense: coarse.two_level_preconditioner(solver, a, dense)) if two \
            else (lambda dense: preconditioner(solver, dense))
        _cache[key] = [fgmres_single(a, b, minv, restart, tol, 200, cgs2)
                       for minv in (make(False), make(True)) for cgs2 in (True, False)]
    return _cache[key]


def relative_to_cycle_start(hist, ref_hist, ref_starts, upto):
    """|hist[k] - ref_hist[k]| / (the reference's start residual of the cycle entry k belongs to), k = 1 .. upto."""
    out = []
    for k in range(1, upto + 1):
        start = [v for ks, v in ref_starts if ks < k][-1]
        out.append(abs(hist[k] - ref_hist[k]) / start)
    return np.array(out)


def parity(schwz, name, kind, settings, restart, two=False):
    _, out = device_run(schwz, kind, settings, restart=restart, two=two)
    runs = references(schwz, kind, settings, restart, 1e-8, two)
    ref_hist, ref_apps, _, ref_starts = runs[0]
    first_cycle = restart == 30
    lengths = [len(h) for h, _, _, _ in runs] + [len(out["history"])]
    # (the first cycle ends where the reference's second one starts: at the provisional stop, or at `restart`)
    ends = [r[3][1][0] for r in runs] + [out["cycle_starts"][1][0]]
    # (where the runs do not all end it at the same entry, that entry is recomputed in some and recurred in others)
    upto = (min(ends) - (len(set(ends)) > 1)) if first_cycle else min(lengths) - 1
    spread = max(float(relative_to_cycle_start(ha, hb, ref_starts, upto).max()) for ha, _, _, _ in runs
                 for hb, _, _, _ in runs)
    dev = float(relative_to_cycle_start(np.array(out["history"]), ref_hist, ref_starts, upto).max())
    log("outer FGMRES, fp32 basis, parity %s (restart %d, %s, %d entries): spread of the four host variants %.3e, device "
        "against CGS2/SuperLU %.3e (margin %.3e), applications device %d / host %s"
        % (name, restart, "first cycle" if first_cycle else "all cycles", upto, spread, dev, 10 * spread,
           out["iter_count"], [r[1] for r in runs]))
    assert out["converged"] and upto >= 5
    assert len(out["history"]) == out["iter_count"] + 1
    if not first_cycle:
        assert len(out["cycle_starts"]) > 2 and [k for k, _ in out["cycle_starts"][:3]] == [0, 5, 10]
    assert dev <= 10 * spread, (dev, spread)


def test_parity_cholmod_ras(schwz):
    parity(schwz, "cholmod / ras", "laplacian", CHOLMOD, 30)


def test_parity_pivoted_lu_on_convection(schwz):
    parity(schwz, "umfpack / convection", "convection", UMFPACK, 30)


def test_parity_two_level(schwz):
    parity(schwz, "cholmod / two-level", "laplacian", CHOLMOD, 30, two=True)


def test_parity_restart_five(schwz):
    parity(schwz, "cholmod / ras", "laplacian", CHOLMOD, 5)


# ---- the truth of the answer ------------------------------------------------------------------------------------------

def check_truth(out, kind, tol, converged=True):
    a, b = matrix(kind), rhs()
    x = out["solution"]
    assert out["converged"] is converged or bool(out["converged"]) == converged
    if converged:
        assert out["history"][-1] <= tol * np.linalg.norm(b)
    al = a.tocsr()
    r = b.astype(LD) - np.array([np.sum(al.data[al.indptr[i]:al.indptr[i + 1]].astype(LD)
                                        * x[al.indices[al.indptr[i]:al.indptr[i + 1]]].astype(LD)) for i in range(N)])
    true = float(np.sqrt(np.sum(r * r)))
    bound = (int(np.diff(al.indptr).max()) + 2) * 2.0 ** -52 * float(np.linalg.norm(np.abs(b) + abs(al) @ np.abs(x)))
    print("true residual %.6e, history[-1] %.6e, difference %.3e, bound %.3e" % (true, out["history"][-1],
                                                                                abs(true - out["history"][-1]), bound))
    assert abs(true - out["history"][-1]) <= bound, (true, out["history"][-1], bound)
    starts = out["cycle_starts"]
    assert starts[0] == (0, out["history"][0]) and starts[-1] == (out["iter_count"], out["history"][-1])
    for (k0, v0), (k1, v1) in zip(starts, starts[1:]):
        assert k1 > k0 and v1 <= v0, starts
        assert out["history"][k1] == v1  # every cycle end is a recomputed residual


@pytest.mark.parametrize("two", [False, True], ids=["ras", "two-level"])
@pytest.mark.parametrize("tol", [1e-8, 1e-12])
def test_truth_of_the_answer_and_counts(schwz, tol, two):
    _, out = device_run(schwz, "laplacian", CHOLMOD, tol=tol, two=two)
    check_truth(out, "laplacian", tol)
    # counts: within +-1 of the range the four host variants span, not below the double basis
    host = [r[1] for r in references(schwz, "laplacian", CHOLMOD, 30, tol, two)]
    _, double = device_run(schwz, "laplacian", CHOLMOD, basis="double", tol=tol, two=two)
    log("outer FGMRES, fp32 basis, applications (%s, tolerance %g): device %d, host variants %s, double-basis device %d "
        "(difference %d); cycles %s" % ("two-level" if two else "ras", tol, out["iter_count"], host, double["iter_count"],
                                        out["iter_count"] - double["iter_count"],
                                        [(k, "%.2e" % v) for k, v in out["cycle_starts"]]))
    assert double["converged"]
    assert min(host) - 1 <= out["iter_count"] <= max(host) + 1
    assert out["iter_count"] >= double["iter_count"]


# ---- other cases ------------------------------------------------------------------------------------------------------

def test_flexible_with_ten_cg_iterations(schwz):
    _, out = device_run(schwz, "laplacian", {}, **JACOBI_CG10)
    assert out["iter_count"] < 200
    check_truth(out, "laplacian", 1e-8)


def test_capped_in_mid_cycle(schwz):
    _, out = device_run(schwz, "laplacian", CHOLMOD, max_iters=7)
    assert out["iter_count"] == 7 and len(out["history"]) == 8 and out["cycle_starts"][-1][0] == 7
    check_truth(out, "laplacian", 1e-8, converged=False)
    assert out["residual_norm"] == pytest.approx(out["history"][-1], rel=1e-10)


def test_double_given_explicitly_is_the_default(schwz):
    _, given = device_run(schwz, "laplacian", CHOLMOD, basis="double", max_iters=7)
    _, default = device_run(schwz, "laplacian", CHOLMOD, basis=None, max_iters=7)
    assert np.array(given["history"]).tobytes() == np.array(default["history"]).tobytes()
    assert given["solution"].tobytes() == default["solution"].tobytes()
    assert given["cycle_starts"] == default["cycle_starts"] and given["iter_count"] == default["iter_count"] == 7


def test_state_hygiene_and_switching(schwz):
    """After a "single" run the solver is an ordinary one again: a stationary solve(b, "zero") is bit for bit a fresh
    solver's; and one solver switched single -> double -> single gives, run by run, the bytes of fresh solvers.  (Every
    run is capped at a few outer iterations: what is compared are bits.)"""
    b = rhs()
    _, fresh_single = device_run(schwz, "laplacian", CHOLMOD, max_iters=7)
    _, fresh_double = device_run(schwz, "laplacian", CHOLMOD, basis="double", max_iters=7)
    solver = make_solver(schwz, "laplacian", CHOLMOD, max_iters=7, outer_basis="single")
    for basis, fresh in (("single", fresh_single), ("double", fresh_double), ("single", fresh_single)):
        solver.metadata.outer_basis = basis
        got = solver.solve(b, "zero")
        assert solver._outer["obj"].basis == basis
        assert np.array(got["history"]).tobytes() == np.array(fresh["history"]).tobytes(), basis
        assert got["solution"].tobytes() == fresh["solution"].tobytes(), basis
        assert got["cycle_starts"] == fresh["cycle_starts"]
    solver.metadata.outer_iteration, solver.metadata.max_iters = "richardson", 6
    again = solver.solve(b, "zero")
    ref_solver = make_solver(schwz, "laplacian", CHOLMOD, outer="richardson", max_iters=6)
    ref = ref_solver.run()
    assert again["iter_count"] == ref["iter_count"] == 6 and again["converged"] == ref["converged"]
    assert again["solution"].tobytes() == ref["solution"].tobytes()
    assert again["residual_norm"] == ref["residual_norm"]
    ppd_a, ppd_r = solver.metadata.post_process_data, ref_solver.metadata.post_process_data
    assert len(ppd_r["local_residual_vector_out"]) == 6 * P
    assert ppd_a["local_residual_vector_out"] == ppd_r["local_residual_vector_out"]
    assert ppd_a["global_residual_vector_out"] == ppd_r["global_residual_vector_out"]
