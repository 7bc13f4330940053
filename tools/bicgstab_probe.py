"""BiCGSTAB (csrc/bicgstab.hip) against GMRES(restart_iter = 1, 30) (csrc/gmres.hip) as stand-alone solvers on one
GPU: convection_diffusion_2d(n) of tests/conftest.py (default n = 1024: 1 M rows), scalar Jacobi, x_0 = 0, and two
right-hand sides: seeded standard normal values ("random") and b = 1 ("ones").  b = 1 is the hard case for BiCGSTAB:
the shadow residual rhat = r_0 = b is then a constant vector, which the interior rows of a convection-diffusion matrix
(row sums zero) annihilate, so rhat.v is carried by the boundary rows alone.

  1. time per iteration and per matrix-vector product of a fixed number of iterations (rtol = 0, no statistics
     asked for; the host polls the device state one batch of iterations / one cycle behind the launches).  The
     three solvers run in ONE process in alternating blocks, every
     timed solve between two device events, the figure the median over all timed solves of a solver.  Products:
     BiCGSTAB 2 per iteration + the start residual; GMRES 1 per Krylov vector + 1 residual per cycle.
  2. time, iterations and products to a 1e-6 reduction of the TRUE residual ||b - A x|| / ||b||, computed outside
     the solvers with schwz_csr_spmv.  Every solver stops on its own (recurred / rotated) norm; where that leaves
     the true residual above the target the solve is repeated from x_0 with rtol tightened by the miss.  A solver
     that does not get there within --max-iters, or that ends in a breakdown, says so, with the reduction it
     reached.
  3. device memory of each solver object (hipMemGetInfo before and after its creation; the preconditioner included).

No threshold hangs on these numbers.

  python tools/bicgstab_probe.py [--n 1024] [--iters 60] [--blocks 3] [--solves 5] [--max-iters 20000] [--fixed-only] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "schwarz-lib_amd"), os.path.join(ROOT, "tests")]


def products(name, iters, restart):
    if name == "bicgstab":
        return 2 * iters + 1
    return iters + (iters + restart - 1) // restart


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=20000)
    ap.add_argument("--fixed-only", action="store_true", help="part 1 alone (for a run under a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import schwz_amd as schwz
    from conftest import convection_diffusion_2d
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rp, col, val = convection_diffusion_2d(args.n)
    n = len(rp) - 1
    A = schwz.Csr(rp, col, val)
    nnz = int(rp[-1])
    say("convection_diffusion_2d(%d): %d rows, %d nonzeros, format %d, scalar Jacobi, %s" %
        (args.n, n, nnz, A.format(), torch.cuda.get_device_name(0)))

    def mem():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    solvers = {}
    for name, restart in (("bicgstab", 0), ("gmres1", 1), ("gmres30", 30)):
        before = mem()
        obj = schwz.Bicgstab(A, schwz.capi.PRECOND_JACOBI, 1) if restart == 0 else \
            schwz.Gmres(A, schwz.capi.PRECOND_JACOBI, 1, restart)
        used = before - mem()
        solvers[name] = (obj, restart)
        say("  %-9s object: %8.1f MB of device memory = %.1f vectors of n doubles" % (name, used / 1e6, used / (8.0 * n)))

    rhs = {"random": torch.from_numpy(np.random.default_rng(29).standard_normal(n)).cuda(),
           "ones": torch.ones(n, dtype=torch.float64, device="cuda")}
    d_b = rhs["random"]
    d_x = torch.zeros(n, dtype=torch.float64, device="cuda")
    d_r = torch.zeros(n, dtype=torch.float64, device="cuda")

    def true_reduction(d_b):
        A.spmv(d_x.data_ptr(), d_r.data_ptr())
        torch.cuda.synchronize()
        return float(torch.linalg.norm(d_b - d_r)) / float(torch.linalg.norm(d_b))

    # ---- 1. fixed iteration counts, alternating blocks ----
    say()
    say("fixed work: %d iterations per solve, %d blocks x %d timed solves per solver, alternating" %
        (args.iters, args.blocks, args.solves))
    times = {name: [] for name in solvers}
    for _ in range(args.blocks):
        for name, (obj, restart) in solvers.items():
            for k in range(args.solves + 1):          # the first solve of a block warms up
                d_x.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                obj.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, args.iters, want_stats=False)
                e1.record()
                torch.cuda.synchronize()
                if k:
                    times[name].append(e0.elapsed_time(e1))
    for name, (obj, restart) in solvers.items():
        t = statistics.median(times[name])
        nprod = products(name, args.iters, max(restart, 1))
        say("  %-9s %8.3f ms per solve (min %.3f, max %.3f)  %7.2f us per iteration  %7.2f us per product (%d products)" %
            (name, t, min(times[name]), max(times[name]), 1e3 * t / args.iters, 1e3 * t / nprod, nprod))

    # ---- 2. to a 1e-6 reduction of the true residual ----
    target = 1e-6
    for which, d_b in ({} if args.fixed_only else rhs).items():
        bnorm = float(torch.linalg.norm(d_b))
        say()
        say("rhs %s: to ||b - A x|| <= 1e-6 ||b|| (true residual), at most %d iterations" % (which, args.max_iters))
        for name, (obj, restart) in solvers.items():
            rtol = target
            for attempt in range(4):
                d_x.zero_()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                it, rn = obj.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, args.max_iters)
                e1.record()
                torch.cuda.synchronize()
                red = true_reduction(d_b)
                ms = e0.elapsed_time(e1)
                flag = obj.breakdown() if name == "bicgstab" else 0
                # repeat with a tighter rtol only where the solver met its own test and the true residual lags
                if red <= target or it >= args.max_iters or flag or rn > rtol * bnorm:
                    break
                rtol *= 0.5 * target / red
            nprod = products(name, it, max(restart, 1))
            verdict = "reached" if red <= target else ("BREAKDOWN %d" % flag if flag else "NOT reached")
            say("  %-9s %s: %6d iterations, %6d products, %9.2f ms, reported %.3e, true reduction %.3e "
                "(rtol %.2e, %d solve%s)" % (name, verdict, it, nprod, ms, rn / bnorm, red, rtol, attempt + 1,
                                             "" if attempt == 0 else "s"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
