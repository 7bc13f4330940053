"""What solving again on a set-up solver saves (SolverRAS.set_rhs / solve, csrc/rhs.hip): the N^3 Laplacian (256),
Jacobi-CG(10) with local_tol 0, tolerance 1e-8, on 1, 2, 4 and 8 in-process subdomains (z-slabs) of one GPU, with one
level and with two (boxes of 16^3 rows as aggregates).

Per configuration, wall time with the device synchronised at both ends:
  initialize()                      the whole setup, and of it the coarse plan (aggregate exchange, plan, upload, A0^-1)
  set_rhs(host array)               new b through _rhs_first_rows + one copy per subdomain, beta, restart
  set_rhs(device tensor)            new b gathered on the device (the first call uploads the index map: shown apart)
then five right-hand sides solved both ways -- five fresh solvers (initialize + run) against one solver
(initialize + run, four times solve) -- with the iteration counts, which must agree pair by pair, and the totals.

  python tools/resolve_probe.py [--n 256] [--subdomains 1,2,4,8] [--box 16] [--levels 1,2] [--rhs 5] [--max-iters 3000]
                                [--out FILE]"""
import argparse
import gc
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def boxes(n, b, P):
    """Aggregate id per row (natural ordering) for cubes of b^3 rows; None where they do not fit the P z-slabs."""
    if n % P or (n // P) % b or n % b:
        return None
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    c = n // b
    return (((z // b) * c + y // b) * c + x // b).reshape(-1).astype(np.int64)


def make(schwz, n, P, agg, max_iters):
    kw = dict(tolerance=1e-8, max_iters=max_iters, local_precond="block-jacobi", precond_max_block_size=1,
              local_solver_tolerance=0.0, local_max_iters=10, num_subdomains=P)
    if agg is not None:
        kw.update(coarse_space="aggregates", coarse_aggregate_vector=agg)
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(n, n, n), overlap=2)
    return schwz.SolverRAS(s, schwz.Metadata(**kw), comm=schwz.InProcessComm(P), quiet=True)


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--subdomains", default="1,2,4,8")
    ap.add_argument("--box", type=int, default=16)
    ap.add_argument("--levels", default="1,2")
    ap.add_argument("--rhs", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=3000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "schwarz-lib_amd"))
    import torch
    import schwz_amd as schwz
    out = open(a.out, "w") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    n, N = a.n, a.n ** 3
    rng = np.random.default_rng(24)
    rhs = [rng.uniform(0.5, 1.5, N) for _ in range(a.rhs)]
    say("# resolve_probe: %d^3 Laplacian, Jacobi-CG(10), tolerance 1e-8, %d right-hand sides, %s" %
        (n, a.rhs, torch.cuda.get_device_name(0)))
    for levels in [int(v) for v in a.levels.split(",")]:
        for P in [int(v) for v in a.subdomains.split(",")]:
            agg = boxes(n, a.box, P) if levels == 2 else None
            if levels == 2 and (agg is None or int(agg.max()) + 1 > schwz.capi.COARSE_MAX_DOFS):
                say("levels 2 P %d: boxes of %d^3 do not fit (skipped)" % (P, a.box))
                continue
            tag = "levels %d P %d" % (levels, P)
            # ---- the calls, one by one
            solver = make(schwz, n, P, agg, a.max_iters)
            t_init, _ = timed(torch, lambda: solver.initialize(rhs=rhs[0]))
            plan = solver._coarse["setup_seconds"] if getattr(solver, "_coarse", None) else 0.0
            t_host = [timed(torch, lambda: solver.set_rhs(rhs[1]))[0] for _ in range(3)]
            d_b = torch.from_numpy(rhs[2]).cuda()
            t_dev = [timed(torch, lambda: solver.set_rhs(d_b))[0] for _ in range(4)]
            t_keep, _ = timed(torch, lambda: solver.set_rhs(d_b, "keep"))
            say("%s: initialize %.3f s (coarse plan %.3f s) | set_rhs host %s ms | set_rhs device first %.1f ms then %s ms | "
                "keep %.1f ms" % (tag, t_init, plan, " ".join("%.1f" % (1e3 * t) for t in t_host), 1e3 * t_dev[0],
                                   " ".join("%.1f" % (1e3 * t) for t in t_dev[1:]), 1e3 * t_keep))
            del d_b
            # ---- five solves on one solver (the solver above: set up once)
            t_re, its_re, secs_re = 0.0, [], []
            for k, b in enumerate(rhs):
                t, res = timed(torch, lambda: solver.solve(b, gather_solution=False))
                t_re += t
                its_re.append(res["iter_count"])
                secs_re.append(res["elapsed"])
            solver.close()
            del solver
            gc.collect()
            # ---- five fresh solvers
            t_fresh, its_fresh = 0.0, []
            for b in rhs:
                fresh = make(schwz, n, P, agg, a.max_iters)

                def whole():
                    fresh.initialize(rhs=b)
                    return fresh.run(gather_solution=False)
                t, res = timed(torch, whole)
                t_fresh += t
                its_fresh.append(res["iter_count"])
                fresh.close()
                del fresh
                gc.collect()
            say("%s: %d solves: one solver %.3f s (+ its initialize %.3f s) | fresh solvers %.3f s | iterations %s / %s%s | "
                "time to residual per solve %s s" %
                (tag, a.rhs, t_re, t_init, t_fresh, its_re, its_fresh, "" if its_re == its_fresh else "  <-- DIFFER",
                 " ".join("%.3f" % t for t in secs_re)))
    if out:
        out.close()


if __name__ == "__main__":
    main()
