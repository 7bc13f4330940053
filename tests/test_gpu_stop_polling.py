"""The host stops launching once a tolerance stop has been seen, for each of the five iterative solvers.

Launches past a stop return at once, so a solve whose host never looks at the device state still returns the right x
and the right iteration count: `0 < iters < cap` cannot tell a poll that fires from one that does not.  Time can.
With a poll the host launches at most stop + 16 + 32 + 64 + 64 iterations (CG, fp32 CG, Chebyshev), stop + two
restart cycles (GMRES) or stop + two polling batches (BiCGSTAB) whatever max_iters is: a solve capped at 8192 takes as
long as one capped at 256.  Without it the launches grow 32-fold.  The bound is the geometric middle of the two
outcomes, sqrt(32); the same two caps with rtol = 0, where nothing can stop the launches, must lie above it -- the
control that shows the clock can see unstopped work.  BiCGSTAB's control takes the caps 8 and 256, 32-fold apart like
the others: its host polls whatever rtol is, and the device ends a solve without a tolerance by itself once the recurred
residual is exactly zero or a breakdown is flagged, which on this matrix happens near iteration 300 -- between the
caps 256 and 8192 the polling host stops launching there (ratio 1.4), which is the behaviour under test, not its absence.

rtol comes from the extended-precision restatement alone, on the CPU: rtol * nu is the geometric mean of the norm that
is to stop the solve -- after 20 to 40 iterations -- and the smallest norm any earlier test of the solver saw, the two
at least a factor GAP apart (rounding moves these norms by about 1e-13 relative; in the fp32 solve by about 1e-5).
The GMRES(10) history on this matrix falls by 3.5 to 5 % per Krylov vector between 20 and 40: its gap is 1.03, still
eleven orders of magnitude above the rounding.

Ratios t(8192) / t(256) on an MI355X, minimum of 5 solves each (profiles/r19_solver_state.txt; the bound is 5.66):
0.77 to 1.53 with a tolerance, 25 to 32 for the controls -- with the library before the solvers shared their polling
and with the one after it.

Skips: no extended precision (hp.require_extended_precision), nothing else."""
import time

import numpy as np
import pytest

import cg_child as cc
import hp_bicgstab
import hp_chebyshev
import hp_reference as hp

pytestmark = pytest.mark.gpu

LD = np.longdouble
GAP = {"gmres": 1.03}      # every other solver: 1.2, the gap of test_gpu_chebyshev.py and test_gpu_bicgstab.py
CAPS = (256, 8192)
BOUND = float(np.sqrt(CAPS[1] / CAPS[0]))
CONTROL_CAPS = {"bicgstab": (8, 256)}      # every other solver: CAPS
STOP_RANGE = (20, 40)
RESTART = 10
CHEB_BOUNDS = (0.025, 2.0)      # of D^-1 A on the 12 x 12 x 12 Laplacian (test_gpu_streams.py)
SOLVERS = ["cg", "cg_f32", "chebyshev", "gmres", "bicgstab"]


def _pick_stop(tests, nu, gap):
    """tests: (norm, iteration count the solve reports when this test stops it) in the order the solver tests them.
    Returns (rtol, count) of the test with the widest gap to every earlier norm among those with a count in
    STOP_RANGE."""
    best = None
    low = float("inf")
    for norm, count in tests:
        norm = float(norm)
        if STOP_RANGE[0] <= count <= STOP_RANGE[1] and norm > 0.0 and norm * gap <= low:
            if best is None or low / norm > best[0]:
                best = (low / norm, float(np.sqrt(norm * low) / float(nu)), count)
        low = min(low, norm)
    assert best is not None, "no clear gap between iterations %d and %d: take another right-hand side" % STOP_RANGE
    return best[1], best[2]


def _restatement(oracle, convdiff, solver):
    """On the CPU: (matrix, b, x0, rtol, the iteration count the restatement stops at, slack of the device's count)"""
    last = STOP_RANGE[1]
    if solver in ("gmres", "bicgstab"):
        rp, col, val = convdiff(40)
    else:
        rp, col, val = oracle.laplacian3d(12, 12, 12)
        rp, col, val = np.asarray(rp, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64)
    n = len(rp) - 1
    b, x0 = cc.rhs(n, 29)
    M = hp.precond_jacobi(rp, col, val, LD)
    slack = 0
    if solver == "cg":
        _, h = hp.pcg(rp, col, val, b, x0, M, last, 0.0, LD)
        tests = [(v, k) for k, v in enumerate(h)]
    elif solver == "cg_f32":
        # the correction form: CG on A e = r0 / nu from e = 0, whose residual norms are relative to nu
        r0 = np.asarray(b, dtype=LD) - hp.spmv(rp, col, val, x0, LD)
        nu = np.sqrt(hp.dot(r0, r0))
        _, h = hp.pcg(rp, col, val, r0 / nu, None, M, last, 0.0, LD)
        tests = [(v, k) for k, v in enumerate(h)]
        slack = 1                   # fp32 rounding against the longdouble history (test_gpu_mixed.py allows the same)
    elif solver == "chebyshev":
        diag = hp_chebyshev.diagonal(rp, col, val)
        _, h = hp_chebyshev.chebyshev(rp, col, val, b, x0, diag, CHEB_BOUNDS[0], CHEB_BOUNDS[1], last, 0.0, LD)
        tests = [(h[k], k) for k in range(0, last + 1, hp_chebyshev.CHECK_EVERY)]     # the checked iterates
    elif solver == "gmres":
        _, h = hp.gmres(rp, col, val, b, x0, M, last, RESTART, 0.0, LD)
        # (a cycle top tests the true residual, not the rotated right-hand side: those counts are left out)
        tests = [(v, k if k % RESTART else -1) for k, v in enumerate(h)]
    else:
        _, h, hh, bd = hp_bicgstab.bicgstab(rp, col, val, b, x0, M, last, 0.0, LD)
        assert bd == 0 and len(h) - 1 == last
        # top 0, half 0, top 1, half 1, ...: a stop in the half step of iteration k reports k + 1
        tests = []
        for k in range(last):
            tests += [(h[k], k), (hh[k], k + 1)]
    rtol, count = _pick_stop(tests, tests[0][0], GAP.get(solver, 1.2))
    assert 0.0 < rtol < 1.0
    return (rp, col, val), b, x0, rtol, count, slack


def _device_solver(schwz, A, solver):
    if solver == "chebyshev":
        s = schwz.Chebyshev(A, 1)
        s.set_bounds(*CHEB_BOUNDS)
        return s
    if solver == "gmres":
        return schwz.Gmres(A, 1, 1, RESTART)
    return {"cg": schwz.Pcg, "cg_f32": schwz.PcgF32, "bicgstab": schwz.Bicgstab}[solver](A, 1)


def _best_of_5(torch, s, d_b, d_x, d_x0, rtol, cap):
    best = float("inf")
    for _ in range(5):
        d_x.copy_(d_x0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, cap, want_stats=False)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


@pytest.mark.parametrize("solver", SOLVERS)
def test_host_stops_launching_after_a_tolerance_stop(schwz, oracle, torch_cuda, convdiff, solver):
    hp.require_extended_precision()
    torch = torch_cuda
    mat, b, x0, rtol, count, slack = _restatement(oracle, convdiff, solver)
    A = schwz.Csr(*mat)
    s = _device_solver(schwz, A, solver)
    d_b, d_x0 = torch.from_numpy(b).cuda(), torch.from_numpy(x0).cuda()
    d_x = d_x0.clone()
    # the solve does stop where the restatement stops, under either cap
    for cap in CAPS:
        d_x.copy_(d_x0)
        its, _ = s.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, cap)
        assert abs(its - count) <= slack and STOP_RANGE[0] <= its <= STOP_RANGE[1], (solver, cap, its, count)
    stopped = [_best_of_5(torch, s, d_b, d_x, d_x0, rtol, cap) for cap in CAPS]
    control = CONTROL_CAPS.get(solver, CAPS)
    assert control[1] == 32 * control[0]
    free = [_best_of_5(torch, s, d_b, d_x, d_x0, 0.0, cap) for cap in control]
    print("stop polling %-9s stop at %2d (rtol %.3e): t(%d) %.3f ms, t(%d) %.3f ms, ratio %.2f; rtol = 0, caps %d and %d: "
          "%.3f ms, %.3f ms, ratio %.2f; bound %.2f"
          % (solver, count, rtol, CAPS[0], stopped[0] * 1e3, CAPS[1], stopped[1] * 1e3, stopped[1] / stopped[0],
             control[0], control[1], free[0] * 1e3, free[1] * 1e3, free[1] / free[0], BOUND))
    assert stopped[1] < BOUND * stopped[0], (solver, stopped)
    assert free[1] > BOUND * free[0], (solver, free)      # the control: unstopped work is visible
