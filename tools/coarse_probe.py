"""One-level against two-level RAS (Metadata.coarse_space = "aggregates", csrc/coarse.hip) at the
time_to_residual_by_subdomains operating point: the N^3 Laplacian (256), Jacobi-CG(10) with local_tol 0, tolerance
1e-8, max_iters 3000, on 1, 2, 4 and 8 in-process subdomains (z-slabs) of one GPU.

Per subdomain count: coarse_space "none" (--repeats fresh runs: their spread is the run-to-run scatter the other
figures are read against), then one run per box shape of --boxes (geometric aggregates handed over as
coarse_aggregate_vector; shapes that give more than 4096 aggregates or do not fit the slabs are skipped and said so).
Per run: outer iterations, milliseconds per step (wall time of the run over its steps), time to residual, the coarse
step's own time per step (device events around residual + solve + apply of every step), the setup seconds of the plan
(aggregate exchange, plan, upload, A0 inverse), and -- from 20 repetitions of each launch kind after the run, between
device events -- the bytes per second of the apply pass and of the GEMV against schwz_ras_algorithmic_bytes(sd, 2)'s
price list (apply: 18 B per slot + 16 B per local row where y is a buffer of its own; GEMV: 8 nc^2 + 16 nc).

  python tools/coarse_probe.py [--n 256] [--subdomains 1,2,4,8] [--boxes 16x16x16,32x32x32] [--repeats 2]
                               [--max-iters 3000]
                               [--pkg DIR] [--out FILE]
--pkg: another checkout's schwarz-lib_amd (the parent commit's, for the A/B of the "none" path; it knows no coarse
space, so only "none" runs)."""
import argparse
import gc
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def boxes(n, box, P):
    """Aggregate id per row (natural ordering), numbered z-layer of boxes after z-layer; None where the boxes do not
    fit the P z-slabs of the regular partition."""
    bx, by, bz = box
    if n % P or (n // P) % bz:
        return None
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    cx, cy = -(-n // bx), -(-n // by)
    return (((z // bz) * cy + y // by) * cx + x // bx).reshape(-1).astype(np.int64)


def run_one(schwz, torch, n, P, agg, out, max_iters=3000):
    kw = dict(tolerance=1e-8, max_iters=max_iters, local_precond="block-jacobi", precond_max_block_size=1,
              local_solver_tolerance=0.0, local_max_iters=10, num_subdomains=P)
    if agg is not None:
        kw.update(coarse_space="aggregates", coarse_aggregate_vector=agg)
    m = schwz.Metadata(**kw)
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(n, n, n), overlap=2)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    t0 = time.perf_counter()
    solver.initialize()
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    events = []
    co = getattr(solver, "_coarse", None)
    if co is not None:
        inner = solver._coarse_step

        def timed(locals_, stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            inner(locals_, stream)
            e1.record()
            events.append((e0, e1))
        solver._coarse_step = timed
    res = solver.run(gather_solution=False)
    torch.cuda.synchronize()
    steps = max(len(solver._timings[0]), 1)
    line = dict(P=P, iters=res["iter_count"], converged=bool(res["converged"]), ms_per_step=1e3 * res["elapsed"] / steps,
                seconds=res["elapsed"], rel_residual=res["residual_norm"] / res["rhs_norm"], setup_s=setup,
                # host-side milliseconds per step of the five timing ids (exchange incl. the coarse step, boundary
                # update, convergence check incl. the wait for the norm, local solve, restriction)
                phase_ms=",".join("%.3f" % (1e3 * float(np.mean(t)) if len(t) else 0.0) for t in solver._timings))
    if co is not None:
        line.update(nc=co["nc"], coarse_ms_per_step=float(np.mean([a.elapsed_time(b) for a, b in events])),
                    plan_setup_s=co["setup_seconds"])
        obj, sds = co["obj"], list(solver.subdomains.values())

        def timed_reps(fn, reps=20):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps
        t_res = timed_reps(lambda: [sd.coarse_residual(obj) for sd in sds])
        t_gemv = timed_reps(lambda: obj.solve())
        t_apply = timed_reps(lambda: [sd.coarse_apply(obj) for sd in sds])
        apply_bytes = sum(18 * (sd.local_size_x + sd.halo_size) + (16 * sd.local_size_x if sd.y_form() != 1 else 0)
                          for sd in sds)
        gemv_bytes = 8 * co["nc"] ** 2 + 16 * co["nc"]
        line.update(residual_us=1e6 * t_res, gemv_us=1e6 * t_gemv, apply_us=1e6 * t_apply,
                    gemv_GBps=gemv_bytes / t_gemv * 1e-9, apply_GBps=apply_bytes / t_apply * 1e-9,
                    coarse_bytes=sum(sd.algorithmic_bytes(2) for sd in sds), y_forms=[sd.y_form() for sd in sds])
    out(line)
    if co is not None:
        solver._coarse_step = inner   # (the wrapper holds the solver: without this its device memory would be freed by
    del solver                        # the cycle collector in the middle of the next run, and hipFree synchronises)
    gc.collect()
    torch.cuda.synchronize()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--subdomains", default="1,2,4,8")
    ap.add_argument("--boxes", default="16x16x16,32x32x32")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--max-iters", type=int, default=3000)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "schwarz-lib_amd"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path[:0] = [a.pkg]
    import torch
    import schwz_amd as schwz
    two_level = hasattr(schwz.Metadata(), "coarse_space")
    fh = open(a.out, "a") if a.out else None

    def out(line):
        txt = " ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in line.items())
        print(txt, flush=True)
        if fh:
            fh.write(txt + "\n")
            fh.flush()
    out(dict(probe="coarse_probe", n=a.n, pkg=os.path.relpath(a.pkg, ROOT), two_level=two_level,
             device=torch.cuda.get_device_name(0)))
    for P in [int(p) for p in a.subdomains.split(",")]:
        for rep in range(a.repeats):
            out(dict(config="none", repeat=rep))
            run_one(schwz, torch, a.n, P, None, out, a.max_iters)
        if not two_level:
            continue
        for spec in a.boxes.split(","):
            box = tuple(int(v) for v in spec.split("x"))
            agg = boxes(a.n, box, P)
            if agg is None or int(agg.max()) + 1 > schwz.capi.COARSE_MAX_DOFS:
                out(dict(config="boxes " + spec, P=P, skipped="does not fit the slabs" if agg is None else "nc > 4096"))
                continue
            out(dict(config="boxes " + spec))
            run_one(schwz, torch, a.n, P, agg, out, a.max_iters)


if __name__ == "__main__":
    main()
