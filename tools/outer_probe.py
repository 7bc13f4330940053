"""The outer FGMRES (Metadata.outer_iteration = "fgmres", schwz_amd/outer.py, csrc/outer.hip) against the stationary
iteration at the time_to_residual_by_subdomains operating point: the N^3 Laplacian (256), Jacobi-CG(10) with local_tol
0, tolerance 1e-8, on 1, 2, 4 and 8 in-process subdomains (z-slabs) of one GPU.

Per subdomain count: "richardson" (the loop as it was; its stop test is the sum of the local residual norms relative to
iteration 0), then "fgmres" with every restart of --restarts (stop test: global 2-norm relative to ||b||).  The two
tests differ, so the comparison is made at EQUAL TRUE RESIDUAL: from the FGMRES history, the first application count
at which its residual is at or below the true relative residual the stationary run ended with, and that count times the
FGMRES run's milliseconds per outer iteration.  Per FGMRES run also: the share of an outer iteration spent in the sweep,
the operator and the orthogonalisation (a second, shorter run with solver.outer_profile set, which synchronises the
device between the three), the TB/s of the three orthogonalisation passes at j = restart - 1 against their byte model
3 * 8 n (j + 2) + 16 n (device events around 10 repetitions), and the device memory the run added.

  python tools/outer_probe.py [--n 256] [--subdomains 1,2,4,8] [--restarts 10,30] [--max-iters 3000]
                              [--profile-iters 60] [--out FILE]"""
import argparse
import gc
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(schwz, n, P, max_iters, **kw):
    m = schwz.Metadata(tolerance=1e-8, max_iters=max_iters, local_precond="block-jacobi", precond_max_block_size=1,
                       local_solver_tolerance=0.0, local_max_iters=10, num_subdomains=P, **kw)
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(n, n, n), overlap=2)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    return solver


def ortho_rate(schwz, torch, o, j, reps=10):
    """Seconds of dots + project_dots + project_dots at column j on whatever the object holds, and the bytes."""
    h = np.zeros(j + 1)
    o.dots(j)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        o.dots(j)
        o.project_dots(j, h)
        o.project_dots(j, h)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps, 3 * 8 * o.n * (j + 2) + 16 * o.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--subdomains", default="1,2,4,8")
    ap.add_argument("--restarts", default="10,30")
    ap.add_argument("--max-iters", type=int, default=3000)
    ap.add_argument("--profile-iters", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "schwarz-lib_amd")]
    import torch
    import schwz_amd as schwz
    fh = open(a.out, "a") if a.out else None

    def out(line):
        txt = " ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in line.items())
        print(txt, flush=True)
        if fh:
            fh.write(txt + "\n")
            fh.flush()
    out(dict(probe="outer_probe", n=a.n, device=torch.cuda.get_device_name(0), max_iters=a.max_iters))
    for P in [int(p) for p in a.subdomains.split(",")]:
        solver = make(schwz, a.n, P, a.max_iters)
        res = solver.run(gather_solution=False)
        rich_rel = res["residual_norm"] / res["rhs_norm"]
        rich = dict(outer="richardson", P=P, iters=res["iter_count"], converged=bool(res["converged"]),
                    ms_per_iter=1e3 * res["elapsed"] / max(res["iter_count"], 1), seconds=res["elapsed"],
                    true_rel_residual=rich_rel)
        out(rich)
        for restart in [int(r) for r in a.restarts.split(",")]:
            torch.cuda.synchronize()
            before = torch.cuda.mem_get_info()[0]
            solver.metadata.outer_iteration, solver.metadata.outer_restart = "fgmres", restart
            solver.metadata.max_iters = a.max_iters
            res = solver.solve(None, "zero", gather_solution=False)
            torch.cuda.synchronize()
            added = before - torch.cuda.mem_get_info()[0]
            hist = np.array(res["history"]) / res["rhs_norm"]
            ms = 1e3 * res["elapsed"] / max(res["iter_count"], 1)
            reached = np.nonzero(hist <= rich_rel)[0]
            k_eq = int(reached[0]) if len(reached) else -1
            line = dict(outer="fgmres", restart=restart, P=P, iters=res["iter_count"], converged=bool(res["converged"]),
                        cycles=len(res["cycle_starts"]), ms_per_iter=ms, seconds=res["elapsed"],
                        true_rel_residual=res["residual_norm"] / res["rhs_norm"], last_history_rel=float(hist[-1]),
                        iters_to_richardson_residual=k_eq,
                        seconds_to_richardson_residual=(k_eq * ms * 1e-3 if k_eq >= 0 else float("nan")),
                        richardson_seconds=rich["seconds"], richardson_iters=rich["iters"],
                        device_MB_added=added / 2.0 ** 20, vectors_of_n=2 * restart + 4)
            # where an outer iteration goes: a shorter run that synchronises between the three parts
            solver.outer_profile = True
            solver.metadata.max_iters = min(a.profile_iters, max(res["iter_count"], 1))
            prof = solver.solve(None, "zero", gather_solution=False)
            solver.outer_profile = False
            tot = sum(prof["profile"].values())
            line.update({"share_" + k: v / tot for k, v in prof["profile"].items()})
            line.update(profiled_ms_per_iter=1e3 * tot / max(prof["iter_count"], 1))
            t, nbytes = ortho_rate(schwz, torch, solver._outer["obj"], restart - 1)
            line.update(ortho_ms_at_last_column=1e3 * t, ortho_TBps=nbytes / t * 1e-12)
            out(line)
        solver.metadata.outer_iteration = "richardson"
        del solver
        gc.collect()
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
