"""Step time of the RAS iteration with the local solve in fp64 ("double") against fp32 CG on the fp64 start residual
("single", Metadata.local_solver_precision), on the general-matrix path:

  lap256    the 256^3 Laplacian with the matrix codings off (SCHWZ_SPMV_PAIR / PATTERN / DICT = 0 for the upload),
            the configuration of bench.py's csr_plain_loop: one subdomain, Jacobi, 10 iterations, local_tol 0
  ani4xR    tests/golden/ani4_crop replicated R times block-diagonally (R = 8: 24648 rows, a launch-bound size;
            R = 512: 1.6 M rows), same local solve

Both precisions run in ONE process on ONE solver per problem: schwz_ras_set_local_precision switches between blocks
of steps (warm-up steps after every switch, every timed step between two device events), the blocks alternate, and
the figure is the median over all timed steps of a precision.  Bytes: schwz_ras_algorithmic_bytes(sd, 1) x
iterations, i.e. the library's price list -- for fp64 SURVEY 8(d)'s generic 12 nnz + 4 (n + 1) + 152 n per iteration
(240 B per row of a 7-point matrix, more than the stored-q kernels really move: 152 B), for fp32 what cg_f32.hip moves
(112 B).  Their quotient over the WHOLE step time is printed as "priced bytes / step time"; it is neither a kernel's
bandwidth nor a ceiling.  The ceiling of the step-time ratio is the quotient of what the kernels move, 152 / 112 = 1.36
(1.6 in the issue's coarser model), printed as such.  Then, on fresh solvers, the outer iterations to a relative residual of 1e-8
(or the residual reached at --max-outer) in both precisions.

  python tools/mixed_probe.py [--problems lap256,ani4x8,ani4x512] [--steps 20] [--blocks 3] [--out FILE]
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


def make_solver(schwz, problem, inner, tol, max_iters, precision):
    """One subdomain, Jacobi, `inner` iterations of the local solve (local_tol 0)."""
    m = schwz.Metadata(tolerance=tol, max_iters=max_iters, local_precond="block-jacobi", precond_max_block_size=1,
                       local_solver_tolerance=0.0, local_max_iters=inner, num_subdomains=1,
                       local_solver_precision=precision)
    if problem == "lap256":
        s = schwz.Settings(laplacian_dim=3, laplacian_shape=(256, 256, 256), overlap=2)
        matrix = None
    else:
        s = schwz.Settings(explicit_laplacian=False, overlap=2)
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
    import torch
    import schwz_amd as schwz
    if not torch.cuda.is_available():
        sys.exit("mixed_probe: no GPU (nothing here can be measured on a CPU)")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("mixed_probe on %s: %d inner iterations, %d blocks x %d timed steps per precision, %d warm-up steps per block"
        % (torch.cuda.get_device_name(0), a.inner, a.blocks, a.steps, a.warmup))
    for problem in [p for p in a.problems.split(",") if p]:
        total = a.blocks * 2 * (a.warmup + a.steps) + 4
        solver, m = make_solver(schwz, problem, a.inner, 1e-30, total, "double")
        sd = solver.subdomains[0]
        solver.begin_run()
        times = {"double": [], "single": []}
        nbytes = {}
        for _ in range(a.blocks):
            for prec, code in (("double", schwz.capi.PRECISION_F64), ("single", schwz.capi.PRECISION_F32)):
                sd.set_local_precision(code)
                nbytes[prec] = a.inner * sd.algorithmic_bytes(1)
                times[prec] += timed_block(solver, torch, a.warmup, a.steps)
        say("%s: %d rows, %d nonzeros" % (problem, sd.local_size_x, sd.nnz_local))
        med = {}
        for prec in ("double", "single"):
            t = times[prec]
            med[prec] = statistics.median(t)
            say("  %-6s ms/step median %.4f  min %.4f  max %.4f  (n = %d)   priced bytes / step time = %.2f TB/s"
                % (prec, med[prec], min(t), max(t), len(t), nbytes[prec] / (med[prec] * 1e-3) / 1e12))
        nnz_row = sd.nnz_local / max(sd.local_size_x, 1)
        moved = (12 * nnz_row + 4 + 64) / (8 * nnz_row + 4 + 52)   # stored-q fp64 kernels over the fp32 kernels
        say("  step time double / single = %.3f   (ceiling from the bytes the iteration kernels move: %.2f)"
            % (med["double"] / med["single"], moved))
        del solver, sd
        torch.cuda.empty_cache()
        for prec in ("double", "single"):
            solver, m = make_solver(schwz, problem, a.inner, 1e-8, a.max_outer, prec)
            out = solver.run(gather_solution=False)
            say("  %-6s outer iterations to 1e-8: %s (relative residual %.3e after %d)"
                % (prec, out["iter_count"] if out["converged"] else "not within %d" % a.max_outer,
                   out["residual_norm"] / out["rhs_norm"], out["iter_count"]))
            del solver
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
