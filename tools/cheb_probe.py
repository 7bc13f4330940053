"""Step time of the RAS iteration with the local solve by CG against the Chebyshev iteration
(Metadata.symmetric_solver = "chebyshev", csrc/chebyshev.hip), on the general-matrix path -- the shapes of
tools/mixed_probe.py:

  lap256    the 256^3 Laplacian with the matrix codings off (SCHWZ_SPMV_PAIR / PATTERN / DICT = 0 for the upload) and
            spmv_variant = 6 (plain CSR): one subdomain, Jacobi, local_tol 0
  ani4xR    tests/golden/ani4_crop replicated R times block-diagonally (R = 8: 24648 rows, a launch-bound size;
            R = 512: 1.6 M rows), same local solve

Both solvers run in ONE process on ONE RAS solver per problem: schwz_ras_set_sym_solver switches between blocks of
steps (warm-up steps after every switch, every timed step between two device events), the blocks alternate, and the
figure is the median over all timed steps of a (solver, inner iteration count) pair.  Every block runs at `--inner`
(10) and at twice as many inner iterations (schwz_ras_set_local_max_iters); the time per inner iteration is the
difference of the two medians over the difference of the counts, i.e. without the step's fixed part (boundary
update, check residual, restriction, the start launches).  Chebyshev runs on its default bounds (Gershgorin bound / 30,
Gershgorin bound).  Bytes: schwz_ras_algorithmic_bytes(sd, 1), the library's price list, over the time per inner
iteration.  Then, on fresh solvers, the outer iterations and the wall time of a run to a relative residual of 1e-8 (or
the residual reached at --max-outer) with each local solver.

  python tools/cheb_probe.py [--problems lap256,ani4x8,ani4x512] [--steps 20] [--blocks 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "schwarz-lib_amd")]
CODINGS = ("SCHWZ_SPMV_PAIR", "SCHWZ_SPMV_PATTERN", "SCHWZ_SPMV_DICT")


def ani4_replicated(rep):
    g = np.load(os.path.join(ROOT, "tests", "golden", "ani4_crop.npz"))
    rp, col, val = g["rp"].astype(np.int64), g["col"].astype(np.int64), g["val"].astype(np.float64)
    n, nnz = len(rp) - 1, int(rp[-1])
    rps = np.concatenate([[0]] + [rp[1:] + k * nnz for k in range(rep)])
    cols = np.concatenate([col + k * n for k in range(rep)]).astype(np.int32)
    return rps, cols, np.tile(val, rep)


def make_solver(schwz, problem, inner, tol, max_iters, local):
    """One subdomain, Jacobi, `inner` iterations of the local solve `local` ("cg" / "chebyshev"; local_tol 0)."""
    m = schwz.Metadata(tolerance=tol, max_iters=max_iters, local_precond="block-jacobi", precond_max_block_size=1,
                       local_solver_tolerance=0.0, local_max_iters=inner, num_subdomains=1, symmetric_solver=local)
    if problem == "lap256":
        s = schwz.Settings(laplacian_dim=3, laplacian_shape=(256, 256, 256), overlap=2, spmv_variant=6)
        matrix = None
    else:
        s = schwz.Settings(explicit_laplacian=False, overlap=2, spmv_variant=6)
        matrix = ani4_replicated(int(problem[5:]))
    s.convergence_settings.enable_global_check = True
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(1), quiet=True)
    saved = {k: os.environ.get(k) for k in CODINGS}
    os.environ.update({k: "0" for k in CODINGS})   # read at the upload of the local matrix
    try:
        solver.initialize(matrix=matrix)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return solver, m


def timed_block(solver, torch, warmup, steps):
    for _ in range(warmup):
        solver.step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        solver.step()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="lap256,ani4x8,ani4x512")
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-outer", type=int, default=400)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import time
    import torch
    import schwz_amd as schwz
    if not torch.cuda.is_available():
        sys.exit("cheb_probe: no GPU (nothing here can be measured on a CPU)")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("cheb_probe on %s: %d and %d inner iterations, %d blocks x %d timed steps per pair, %d warm-up steps per block"
        % (torch.cuda.get_device_name(0), a.inner, 2 * a.inner, a.blocks, a.steps, a.warmup))
    solvers = (("cg", schwz.capi.SYM_CG), ("chebyshev", schwz.capi.SYM_CHEBYSHEV))
    for problem in [p for p in a.problems.split(",") if p]:
        total = a.blocks * 4 * (a.warmup + a.steps) + 4
        solver, m = make_solver(schwz, problem, a.inner, 1e-30, total, "cg")
        sd = solver.subdomains[0]
        solver.begin_run()
        times = {(name, k): [] for name, _ in solvers for k in (1, 2)}
        nbytes = {}
        for _ in range(a.blocks):
            for name, code in solvers:
                sd.set_sym_solver(code)
                nbytes[name] = sd.algorithmic_bytes(1)
                for k in (1, 2):
                    sd.set_local_max_iters(k * a.inner)
                    times[(name, k)] += timed_block(solver, torch, a.warmup, a.steps)
        say("%s: %d rows, %d nonzeros; Chebyshev bounds %r" % (problem, sd.local_size_x, sd.nnz_local, sd.cheb_bounds()))
        per, step = {}, {}
        for name, _ in solvers:
            med = {k: statistics.median(times[(name, k)]) for k in (1, 2)}
            step[name] = med[1]
            per[name] = (med[2] - med[1]) / a.inner
            for k in (1, 2):
                t = times[(name, k)]
                say("  %-9s %2d inner: ms/step median %.4f  min %.4f  max %.4f  (n = %d)"
                    % (name, k * a.inner, med[k], min(t), max(t), len(t)))
            say("  %-9s us per inner iteration %.2f   priced bytes / that time = %.2f TB/s"
                % (name, per[name] * 1e3, nbytes[name] / (per[name] * 1e-3) / 1e12))
        say("  cg / chebyshev: per inner iteration %.3f, per step at %d inner iterations %.3f"
            % (per["cg"] / per["chebyshev"], a.inner, step["cg"] / step["chebyshev"]))
        del solver, sd
        torch.cuda.empty_cache()
        for name, _ in solvers:
            solver, m = make_solver(schwz, problem, a.inner, 1e-8, a.max_outer, name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = solver.run(gather_solution=False)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            say("  %-9s run to 1e-8: %s outer iterations, %.1f ms wall (relative residual %.3e after %d)"
                % (name, out["iter_count"] if out["converged"] else "not within %d" % a.max_outer, wall * 1e3,
                   out["residual_norm"] / out["rhs_norm"], out["iter_count"]))
            del solver
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
