"""Outer FGMRES preconditioned by one RAS sweep or by one two-level step (an extension: the reference's only outer
iteration is the stationary one of SchwarzBase::run, and it has no outer Krylov method).

metadata.outer_iteration = "fgmres" makes SolverRAS.run() -- and with it solve() and a run() after set_rhs() -- a loop
of its own, as solve_many is: right-preconditioned flexible GMRES(outer_restart) on the global system, flexible
because an iterative local solve is no fixed linear operator.  Per outer iteration j

  z_j = M^-1 v_j   one RAS sweep from a zero start with right-hand side v_j, made of the calls of the stationary step:
                   v_j into the interiors of x~, halo exchange (every other slot of x~ from its owner), rhs_set from
                   the device address of x~, restart(keep_x=False), local_solve, restrict; the interior of x~ is z_j
  w = A z_j        a second exchange, then schwz_ras_apply_interior
  orthogonalise    classical Gram-Schmidt applied twice on the device (core.Outer: dots, project_dots twice), the norm
                   of the result by a reduction
  Givens + solve   on the host in float64 (GivensLeastSquares below)

With metadata.outer_preconditioner = "two-level" (and coarse_space = "aggregates") z_j is the stationary two-level step
from a zero start with the right-hand side v_j, the coarse correction first and the sweep on the corrected residual:

  z0 = Z A0^-1 Z^T v_j,   z_j = z0 + RAS(v_j - A z0)

as: v_j into x~, exchange, rhs_set, aggregate_sums from the vector of id 3 (s = Z^T v_j: the streaming restriction -- beta
of the coarse plan belongs to the caller's b and is neither used nor touched), the coarse solve once, then per subdomain
restart(keep_x=False), coarse_apply (x~ = y = c[agg] on every slot, halo included: no second exchange),
update_boundary (b~ = v_j - A_Gamma z0 on the overlap rows), local_solve from the warm start y = z0, restrict.  The
additive form RAS(v) + z0 is not offered: with unsmoothed aggregates it needed as many applications as one level.

and at the end of a cycle x += sum y_i Z_i, the true residual recomputed for the next cycle's v_0.  Two exchanges per
outer iteration where the stationary step has one.  The loop borrows x~, b, b~, y and the solver objects of the
subdomains and puts back the caller's b, the solution in x~ (exchanged) and a warm start y = x~.

The stop test is on the GLOBAL 2-norm, history[k] <= tolerance * ||b||_2 -- not the stationary loop's test (the sum of
the local residual norms relative to its value at iteration 0).  Counts of the two loops compare at equal true residual
only.
"""
import math
import time

import numpy as np

from . import _capi as capi
from . import core

OUTER_ITERATIONS = ("richardson", "fgmres")
OUTER_PRECONDITIONERS = ("ras", "two-level")
OUTER_BASES = ("double", "single")


def wants_fgmres(settings, metadata, comm):
    """The four Metadata fields checked (ERR_INVALID) and, for "fgmres", the configurations the loop does not exist for
    refused (NotImplementedSchwz).  Touches neither the backend nor a subdomain.  True: run() is the loop below."""
    name = getattr(metadata, "outer_iteration", "richardson")
    if not isinstance(name, str) or name not in OUTER_ITERATIONS:
        raise capi.SchwzError(capi.ERR_INVALID, "outer_iteration must be 'richardson' or 'fgmres', not %r" % (name,))
    restart = getattr(metadata, "outer_restart", 30)
    if isinstance(restart, bool) or not isinstance(restart, (int, np.integer)) or restart < 1 \
            or restart > capi.OUTER_MAX_RESTART:
        raise capi.SchwzError(capi.ERR_INVALID, "outer_restart must be an integer in 1..%d, not %r"
                              % (capi.OUTER_MAX_RESTART, restart))
    pre = getattr(metadata, "outer_preconditioner", "ras")
    if not isinstance(pre, str) or pre not in OUTER_PRECONDITIONERS:
        raise capi.SchwzError(capi.ERR_INVALID, "outer_preconditioner must be 'ras' or 'two-level', not %r" % (pre,))
    basis = getattr(metadata, "outer_basis", "double")
    if not isinstance(basis, str) or basis not in OUTER_BASES:
        raise capi.SchwzError(capi.ERR_INVALID, "outer_basis must be 'double' or 'single', not %r" % (basis,))
    if name == "richardson":
        return False

    def unavailable(what):
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "outer_iteration 'fgmres' does not exist for " + what)
    coarse = getattr(metadata, "coarse_space", "none")
    if pre == "two-level" and coarse == "none":
        raise capi.SchwzError(capi.ERR_INVALID, "outer_preconditioner 'two-level' needs coarse_space 'aggregates'")
    if pre == "ras" and coarse != "none":
        unavailable("coarse_space '%s' with outer_preconditioner 'ras' (beta of the coarse plan depends on the "
                    "right-hand side): set outer_preconditioner = 'two-level'" % coarse)
    if settings.comm_settings.enable_onesided:
        unavailable("enable_onesided")
    if settings.comm_settings.enable_overlap:
        unavailable("enable_overlap")
    if settings.use_mixed_precision:
        unavailable("use_mixed_precision (fp32 halos)")
    if settings.reset_local_crit_iter != -1:
        unavailable("reset_local_crit_iter (the two-stage local criterion)")
    if comm.size > len(comm.local_ranks):
        unavailable("more than one rank process (the reductions would need a vector all-gather)")
    return True


class GivensLeastSquares:
    """min_y || beta e_1 - H y ||_2 for the (k + 1) x k upper Hessenberg matrix H that grows by a column per outer
    iteration: the Givens rotations applied as the columns arrive, the residual norm |g[k]| after each, and the
    triangular solve, all in float64 on the host."""

    def __init__(self, m, beta):
        self.R = np.zeros((m + 1, m))
        self.cs, self.sn = np.zeros(m), np.zeros(m)
        self.g = np.zeros(m + 1)
        self.g[0] = beta
        self.k = 0

    def append(self, column):
        """column: the k + 2 entries H[0:k+2, k].  Returns the residual norm of the least-squares problem."""
        k = self.k
        h = np.array(column[:k + 2], dtype=np.float64)
        for i in range(k):
            t = self.cs[i] * h[i] + self.sn[i] * h[i + 1]
            h[i + 1] = -self.sn[i] * h[i] + self.cs[i] * h[i + 1]
            h[i] = t
        c, s = 1.0, 0.0
        if h[k + 1] != 0.0:
            rr = math.hypot(h[k], h[k + 1])
            c, s = h[k] / rr, h[k + 1] / rr
        self.cs[k], self.sn[k] = c, s
        h[k] = c * h[k] + s * h[k + 1]
        h[k + 1] = 0.0
        self.R[:k + 2, k] = h
        self.g[k + 1] = -s * self.g[k]
        self.g[k] = c * self.g[k]
        self.k = k + 1
        return abs(self.g[k + 1])

    def solve(self):
        """y of the k columns so far (back substitution; a zero pivot -- a breakdown on a singular system -- gives 0)."""
        k = self.k
        y = np.zeros(k)
        for i in range(k - 1, -1, -1):
            t = self.g[i] - np.dot(self.R[i, i + 1:k], y[i + 1:])
            y[i] = t / self.R[i, i] if self.R[i, i] != 0.0 else 0.0
        return y


def _exchange(solver, stream):
    """The halo exchange of the stationary step without its early form: pack, exchange, unpack."""
    for me, sd in solver.subdomains.items():
        solver._pack(me, sd, stream)
    solver.comm.exchange(solver._sends, solver._recvs)
    for me, sd in solver.subdomains.items():
        solver._unpack(me, sd, stream)


def _drop_pending(solver):
    """What set_rhs drops: an early exchange and overlapped messages left by an interrupted run are completed, not
    applied."""
    comm = solver.comm
    if getattr(solver, "_early", None) is not None:
        handle, solver._early = solver._early, None
        comm.finish_exchange(handle)
    pending, solver._pending = getattr(solver, "_pending", None), None
    if pending is not None:
        comm.finish_exchange(pending["halo"])
        comm.finish_flags(pending["flags"])


def _state(solver, locals_, n, restart, basis="double"):
    """The device objects of the loop, kept on the solver between runs: core.Outer, the iterate x over the n interior
    rows and a copy of every subdomain's right-hand side."""
    st = getattr(solver, "_outer", None)
    # (all the buffers' sizes follow from it)
    shape = (n, restart, tuple((me, sd.local_size_x) for me, sd in locals_), basis)
    if st is None or st["shape"] != shape:
        be = solver.backend
        obj = core.Outer(n, restart) if basis == "double" else core.Outer(n, restart, basis)
        st = dict(shape=shape, obj=obj, x=be.empty(n),
                  b={me: be.empty(sd.local_size_x) for me, sd in locals_})
        solver._outer = st
    return st


def run_fgmres(solver, gather_solution=True):
    """SolverRAS.run() for outer_iteration = "fgmres".  Returns the dict of finish_run plus history: history[k] is
    ||r_k||_2 over all rows after k applications of the preconditioner, k = 0 .. iter_count -- history[0] and the entry
    that met the stop test at the start of a cycle are recomputed true residuals, the others come from the Givens
    recurrence -- and cycle_starts, the (k, recomputed ||b - A x_k||_2) of every cycle.  A profile dict (seconds in the
    sweep, the operator and the orthogonalisation, each behind a device synchronise) where solver.outer_profile is
    set.

    With metadata.outer_basis = "single" (V in fp32, everything else fp64) the recurrence follows the true residual only
    down to about 2^-24 of the cycle's start residual, so the last entry of EVERY cycle -- the one that met the stop
    test and the one that ran into max_iters included -- is the recomputed b - A x, which is also that cycle's entry of
    cycle_starts; converged is said of a recomputed residual only, and where it misses the tolerance another cycle
    starts from it."""
    s, m, be, comm = solver.settings, solver.metadata, solver.backend, solver.comm
    wants_fgmres(s, m, comm)
    if solver.problem is None or not solver.subdomains:
        raise capi.SchwzError(capi.ERR_INVALID, "run: the solver is not set up: call initialize() first")
    restart, tol, P = int(m.outer_restart), float(m.tolerance), m.num_subdomains
    locals_ = list(solver.subdomains.items())
    stream = be.stream()
    _drop_pending(solver)
    offset, n = {}, 0
    for me, sd in locals_:
        offset[me] = n
        n += sd.local_size
    single = getattr(m, "outer_basis", "double") == "single"
    st = _state(solver, locals_, n, restart, "single" if single else "double")
    o, x = st["obj"], st["x"].data_ptr()
    two_level = getattr(m, "outer_preconditioner", "ras") == "two-level"
    coarse = solver._coarse["obj"] if two_level else None
    profile = dict(sweep=0.0, apply=0.0, ortho=0.0) if getattr(solver, "outer_profile", False) else None
    if profile is not None and two_level:
        profile["coarse"] = 0.0

    def clock(key, t0):
        if profile is not None:
            be.synchronize()
            profile[key] += time.perf_counter() - t0
        return time.perf_counter()

    def interiors_from(base):
        """A vector over the n interior rows (device address) into the interiors of the subdomains' x~."""
        for me, sd in locals_:
            core.outer_copy(sd.local_size, base + 8 * offset[me], sd.vector(0)[0], stream)

    def interiors_to(base):
        for me, sd in locals_:
            core.outer_copy(sd.local_size, sd.vector(0)[0], base + 8 * offset[me], stream)

    def apply_to(base):
        """(A x~) on the interior rows into such a vector; x~ is exchanged first."""
        _exchange(solver, stream)
        for me, sd in locals_:
            sd.apply_interior(base + 8 * offset[me], stream)

    def basis_to_interiors(j):
        """V_j into the interiors of the subdomains' x~ (widened where the basis is fp32)."""
        if not single:
            return interiors_from(o.vector(o.V, j))
        for me, sd in locals_:
            o.basis_read(j, offset[me], sd.local_size, sd.vector(0)[0], stream)

    def true_residual():
        """w = b - A x for the x in the interiors of x~: A x into V_0, b into w, one projection with the coefficient 1
        (the product is exact), whose norm comes with it.  With an fp32 basis: A x into Z_0, which is free wherever the
        residual is taken (before the first cycle, after combine), and one pass w = b - t with its norm."""
        if single:
            apply_to(o.vector(o.Z, 0))
            return math.sqrt(o.residual(o.vector(o.Z, 0), stream))
        apply_to(o.vector(o.V, 0))
        core.outer_copy(n, o.vector(o.B), o.vector(o.W), stream)
        return math.sqrt(o.project_dots(0, np.ones(1), stream)[1])

    def diverged(*values):
        if any(v != v for v in values):
            raise capi.SchwzError(capi.ERR_DIVERGED, " Rank %d: the outer FGMRES met a NaN in %d iters "
                                  % (comm.rank, m.iter_count))

    solver._timings = [[] for _ in range(5)]
    solver._num_converged = 0
    m.iter_count = 0
    be.synchronize()
    comm.barrier()
    start = time.perf_counter()
    # the caller's b: a copy per subdomain (the sweeps overwrite the subdomains' own), its interiors as one vector
    for me, sd in locals_:
        core.outer_copy(sd.local_size_x, sd.vector(3)[0], st["b"][me].data_ptr(), stream)
        core.outer_copy(sd.local_size, sd.vector(3)[0], o.vector(o.B) + 8 * offset[me], stream)
    core.outer_copy(n, o.vector(o.B), o.vector(o.W), stream)
    bnorm = math.sqrt(o.dots(0, stream)[1])
    # the start vector is whatever x~ holds: zeros after initialize() and set_rhs(..., "zero"), the last iterate after
    # set_rhs(..., "keep")
    interiors_to(x)
    beta = true_residual()
    diverged(bnorm, beta)
    history, cycle_starts = [beta], [(0, beta)]
    converged = tol > 0.0 and beta <= tol * bnorm
    try:
        while not converged and m.iter_count < m.max_iters and beta != 0.0:
            ls = GivensLeastSquares(restart, beta)
            o.start(1.0 / beta, stream)
            for j in range(restart):
                t0 = time.perf_counter()
                # z_j = M^-1 v_j: one RAS sweep from a zero start with the right-hand side v_j
                basis_to_interiors(j)
                _exchange(solver, stream)
                if not two_level:
                    for _, sd in locals_:
                        sd.rhs_set(sd.vector(0)[0], stream)  # (asked for again every time: a restriction swaps the buffers)
                        sd.restart(False, stream)
                else:
                    # z0 = Z A0^-1 Z^T v_j in x~ and y, then the sweep on v_j - A z0 from the warm start z0
                    for _, sd in locals_:
                        sd.rhs_set(sd.vector(0)[0], stream)
                    t0 = clock("sweep", t0)
                    for _, sd in locals_:
                        sd.aggregate_sums(coarse, sd.vector(3)[0], stream)
                    coarse.solve(stream)
                    t0 = clock("coarse", t0)
                    for _, sd in locals_:
                        sd.restart(False, stream)
                    t0 = clock("sweep", t0)
                    for _, sd in locals_:
                        sd.coarse_apply(coarse, stream)
                    t0 = clock("coarse", t0)
                    for _, sd in locals_:
                        sd.update_boundary(stream)
                for _, sd in locals_:
                    sd.local_solve(stream)
                for _, sd in locals_:
                    sd.restrict(stream)
                interiors_to(o.vector(o.Z, j))
                t0 = clock("sweep", t0)
                # w = A z_j
                apply_to(o.vector(o.W))
                t0 = clock("apply", t0)
                # classical Gram-Schmidt twice; the norm of what is left is a reduction of its own
                h1 = o.dots(j, stream)
                h2 = o.project_dots(j, h1, stream)
                h3 = o.project_dots(j, h2, stream)
                diverged(*h1, *h2, *h3)
                hn = math.sqrt(h3[j + 1])
                if hn != 0.0:
                    o.normalize(j, 1.0 / hn, stream)
                clock("ortho", t0)
                est = ls.append(np.append(h1[:j + 1] + h2[:j + 1], hn))
                m.iter_count += 1
                history.append(est)
                diverged(est)
                converged = tol > 0.0 and est <= tol * bnorm
                if converged or hn == 0.0 or m.iter_count >= m.max_iters:
                    break
            # x += sum y_i Z_i, then the true residual: the next cycle's v_0
            o.combine(ls.solve(), x, stream)
            interiors_from(x)
            if single:
                # a stop inside a cycle is provisional: the recurrence follows the true residual down to about 2^-24
                # of the cycle's start and no further.  Every cycle end -- the one that met the stop test and the one
                # that ran into max_iters too -- recomputes b - A x, and only that says "converged"
                beta = true_residual()
                diverged(beta)
                history[-1] = beta
                cycle_starts.append((m.iter_count, beta))
                converged = tol > 0.0 and beta <= tol * bnorm
                continue
            if converged:
                break
            beta = true_residual()
            diverged(beta)
            cycle_starts.append((m.iter_count, beta))
            if tol > 0.0 and beta <= tol * bnorm:
                history[-1], converged = beta, True
    finally:
        # the subdomains get the caller's b back (b~ = b, the solver objects forget the sweeps) and a warm start y = x~;
        # x~ holds the last iterate in its interiors, the tail's exchange spreads it
        _exchange(solver, stream)
        for me, sd in locals_:
            sd.rhs_set(st["b"][me].data_ptr(), stream)
            sd.restart(True, stream)
            px, py = sd.vector(0)[0], sd.vector(2)[0]
            if py and py != px:
                core.outer_copy(sd.local_size_x, px, py, stream)
    be.synchronize()
    comm.barrier()
    elapsed = time.perf_counter() - start
    solver._num_converged = P if converged else 0
    out = solver.finish_run(elapsed, gather_solution)
    out["history"], out["cycle_starts"] = history, cycle_starts
    if profile is not None:
        out["profile"] = profile
    return out
