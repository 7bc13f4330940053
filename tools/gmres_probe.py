"""GMRES(restart_iter = 1, 10, 30) with the fp64 basis against the compressed basis (csrc/gmres.hip,
SCHWZ_GMRES_BASIS_F32: fp32 basis vectors, fp64 arithmetic, blocked CGS2), and BiCGSTAB beside them, as stand-alone
solvers on one GPU: convection_diffusion_2d(n) of tests/conftest.py (default n = 1024: 1 M rows), scalar Jacobi,
x_0 = 0, a seeded standard normal right-hand side.

  1. time per iteration of a fixed number of Krylov vectors (rtol = 0, no statistics asked for; the host looks at the
     device state one cycle behind the launches).  All solvers run in ONE process in alternating blocks, every timed
     solve between two device events, the figure the median over all timed solves of a solver.  With --no-single
     the same measurement runs on a library without the compressed basis (the parent commit through SCHWZ_HIP_LIB).
  2. time, iterations and products to a 1e-6 reduction of the TRUE residual ||b - A x|| / ||b||, computed outside
     the solvers with schwz_csr_spmv.  Every solver stops on its own (recurred / rotated) norm; where that leaves
     the true residual above the target the solve is repeated from x_0 with rtol tightened by the miss.
  3. device memory of each solver object (hipMemGetInfo before and after its creation; the preconditioner included).

No threshold hangs on these numbers.

  python tools/gmres_probe.py [--n 1024] [--iters 60] [--blocks 3] [--solves 5] [--restarts 1,10,30]
                              [--max-iters 20000] [--fixed-only] [--no-single] [--only NAME] [--out FILE]
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
    ap.add_argument("--restarts", default="1,10,30")
    ap.add_argument("--max-iters", type=int, default=20000)
    ap.add_argument("--fixed-only", action="store_true", help="part 1 alone")
    ap.add_argument("--no-single", action="store_true", help="fp64 bases and BiCGSTAB only (a library without the option)")
    ap.add_argument("--only", default=None, help="one solver by name (for a run under a kernel trace)")
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

    kinds = [("bicgstab", 0, None)]
    for m in (int(t) for t in args.restarts.split(",")):
        kinds.append(("gmres%d/double" % m, m, 0))
        if not args.no_single:
            kinds.append(("gmres%d/single" % m, m, 1))
    if args.only:
        kinds = [k for k in kinds if k[0] == args.only]
    jac = schwz.capi.PRECOND_JACOBI
    solvers = {}
    for name, restart, basis in kinds:
        before = mem()
        if restart == 0:
            obj = schwz.Bicgstab(A, jac, 1)
        elif basis:
            obj = schwz.Gmres(A, jac, 1, restart, basis=schwz.capi.GMRES_BASIS_F32)
        else:
            obj = schwz.Gmres(A, jac, 1, restart)
        used = before - mem()
        solvers[name] = (obj, restart)
        say("  %-15s object: %8.1f MB of device memory = %.1f vectors of n doubles" % (name, used / 1e6, used / (8.0 * n)))

    d_b = torch.from_numpy(np.random.default_rng(29).standard_normal(n)).cuda()
    d_x = torch.zeros(n, dtype=torch.float64, device="cuda")
    d_r = torch.zeros(n, dtype=torch.float64, device="cuda")

    def true_reduction():
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
        say("  %-15s %8.3f ms per solve (min %.3f, max %.3f)  %7.2f us per iteration  %7.2f us per product (%d products)" %
            (name, t, min(times[name]), max(times[name]), 1e3 * t / args.iters, 1e3 * t / nprod, nprod))

    # ---- 2. to a 1e-6 reduction of the true residual ----
    target = 1e-6
    if not args.fixed_only:
        bnorm = float(torch.linalg.norm(d_b))
        say()
        say("to ||b - A x|| <= 1e-6 ||b|| (true residual), at most %d iterations" % args.max_iters)
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
                red = true_reduction()
                ms = e0.elapsed_time(e1)
                flag = obj.breakdown() if name == "bicgstab" else 0
                # repeat with a tighter rtol only where the solver met its own test and the true residual lags
                if red <= target or it >= args.max_iters or flag or rn > rtol * bnorm:
                    break
                rtol *= 0.5 * target / red
            nprod = products(name, it, max(restart, 1))
            verdict = "reached" if red <= target else ("BREAKDOWN %d" % flag if flag else "NOT reached")
            say("  %-15s %s: %6d iterations, %6d products, %9.2f ms, reported %.3e, true reduction %.3e "
                "(rtol %.2e, %d solve%s)" % (name, verdict, it, nprod, ms, rn / bnorm, red, rtol, attempt + 1,
                                             "" if attempt == 0 else "s"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
