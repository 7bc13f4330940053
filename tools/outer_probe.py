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

With --coarse-box B (B^3 boxes as the aggregates of coarse_space = "aggregates"; 16 at 256^3 gives nc = 4096) the probe
measures the two-level preconditioner of the outer FGMRES (Metadata.outer_preconditioner = "two-level") instead.  Per
subdomain count: the streaming restriction schwz_ras_aggregate_sums against schwz_ras_rhs_aggregate on the same
right-hand side (microseconds per call of one subdomain between device events, the median of --reps batches of 20 calls
after a warm-up batch, and the TB/s of the restriction's 12 n model); then the stationary two-level loop, the one-level
FGMRES and the two-level FGMRES with every restart of --restarts: applications, ms per application, seconds, and -- the
three stop tests differ -- the applications and seconds of both FGMRES runs to the TRUE relative residual the
stationary two-level run ended with; the shares of the profile (coarse: restriction + coarse solve + apply).

With --basis single the FGMRES runs keep their Krylov basis in fp32 (Metadata.outer_basis = "single"): the byte model
of the three passes is then 3 * (4 n (j + 1) + 8 n) + 16 n, and every line carries the basis, the orthogonalisation's
seconds and milliseconds per outer iteration (from the profiled run) and the device memory the outer object added.
Run the probe once per basis -- on the parent commit for "double" -- in alternating processes to compare.

  python tools/outer_probe.py [--n 256] [--subdomains 1,2,4,8] [--restarts 10,30] [--max-iters 3000]
                              [--profile-iters 60] [--coarse-box 0] [--reps 7] [--basis double|single] [--out FILE]"""
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
    if getattr(o, "basis", "double") == "single":
        return e0.elapsed_time(e1) * 1e-3 / reps, 3 * (4 * o.n * (j + 1) + 8 * o.n) + 16 * o.n
    return e0.elapsed_time(e1) * 1e-3 / reps, 3 * 8 * o.n * (j + 2) + 16 * o.n


def boxes(n, box):
    """Aggregate id per row of the n^3 grid in natural ordering: box^3 cells, numbered z-layer of boxes after z-layer."""
    i = np.arange(n ** 3, dtype=np.int64)
    x, y, z = i % n, (i // n) % n, i // (n * n)
    c = -(-n // box)
    return ((z // box) * c + y // box) * c + x // box


def restriction_rate(torch, sd, coarse, reps, batch=20):
    """Median microseconds per call of aggregate_sums and of rhs_aggregate on one subdomain (device events around
    `batch` calls, `reps` batches after a warm-up batch each), and the bytes of the 12 n model."""
    def timed(call):
        for _ in range(batch):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                call()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / batch)
        return float(np.median(us)), float(min(us)), float(max(us))
    b = sd.vector(3)[0]
    new = timed(lambda: sd.aggregate_sums(coarse, b))
    old = timed(lambda: sd.rhs_aggregate())  # (recomputes beta from the same b: the same bits every time)
    return new, old, 12 * sd.local_size


def two_level_section(schwz, torch, a, out):
    agg = boxes(a.n, a.coarse_box)
    for P in [int(p) for p in a.subdomains.split(",")]:
        solver = make(schwz, a.n, P, a.max_iters, coarse_space="aggregates", coarse_aggregate_vector=agg)
        coarse = solver._coarse["obj"]
        for me, sd in sorted(solver.subdomains.items()):
            if me not in (0, P - 1):
                continue
            new, old, nbytes = restriction_rate(torch, sd, coarse, a.reps)
            out(dict(restriction="aggregate_sums", P=P, subdomain=me, rows=sd.local_size, nc=solver._coarse["nc"],
                     us_per_call=new[0], us_min=new[1], us_max=new[2], TBps_12n=nbytes / new[0] * 1e-6,
                     model_bytes=sd.algorithmic_bytes(3), rhs_aggregate_us_per_call=old[0], rhs_aggregate_us_min=old[1],
                     rhs_aggregate_us_max=old[2], times_faster=old[0] / new[0]))
        res = solver.solve(None, "zero", gather_solution=False)
        level = res["residual_norm"] / res["rhs_norm"]
        out(dict(outer="richardson", levels=2, P=P, iters=res["iter_count"], converged=bool(res["converged"]),
                 ms_per_iter=1e3 * res["elapsed"] / max(res["iter_count"], 1), seconds=res["elapsed"],
                 true_rel_residual=level))
        one = make(schwz, a.n, P, a.max_iters, outer_iteration="fgmres")
        if a.basis != "double":
            one.metadata.outer_basis = solver.metadata.outer_basis = a.basis
        for restart in [int(r) for r in a.restarts.split(",")]:
            for levels, sv in ((1, one), (2, solver)):
                sv.metadata.outer_iteration, sv.metadata.outer_restart = "fgmres", restart
                sv.metadata.outer_preconditioner = "two-level" if levels == 2 else "ras"
                sv.metadata.max_iters = a.max_iters
                sv.solve(None, "zero", gather_solution=False)  # (warm-up: allocations, code objects, graphs)
                res = sv.solve(None, "zero", gather_solution=False)
                hist = np.array(res["history"]) / res["rhs_norm"]
                ms = 1e3 * res["elapsed"] / max(res["iter_count"], 1)
                reached = np.nonzero(hist <= level)[0]
                k_eq = int(reached[0]) if len(reached) else -1
                line = dict(outer="fgmres", basis=a.basis, levels=levels, restart=restart, P=P, iters=res["iter_count"],
                            converged=bool(res["converged"]), cycles=len(res["cycle_starts"]), ms_per_iter=ms,
                            seconds=res["elapsed"], true_rel_residual=res["residual_norm"] / res["rhs_norm"],
                            iters_to_stationary_residual=k_eq,
                            seconds_to_stationary_residual=(k_eq * ms * 1e-3 if k_eq >= 0 else float("nan")))
                sv.outer_profile = True
                sv.metadata.max_iters = min(a.profile_iters, max(res["iter_count"], 1))
                prof = sv.solve(None, "zero", gather_solution=False)
                sv.outer_profile = False
                tot = sum(prof["profile"].values())
                line.update({"share_" + k: v / tot for k, v in prof["profile"].items()})
                line.update(profiled_ms_per_iter=1e3 * tot / max(prof["iter_count"], 1),
                            ortho_seconds=prof["profile"]["ortho"],
                            ortho_ms_per_iter=1e3 * prof["profile"]["ortho"] / max(prof["iter_count"], 1))
                t, nbytes = ortho_rate(schwz, torch, sv._outer["obj"], restart - 1)
                line.update(ortho_ms_at_last_column=1e3 * t, ortho_TBps=nbytes / t * 1e-12)
                out(line)
        del solver, one, coarse
        gc.collect()
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--subdomains", default="1,2,4,8")
    ap.add_argument("--restarts", default="10,30")
    ap.add_argument("--max-iters", type=int, default=3000)
    ap.add_argument("--profile-iters", type=int, default=60)
    ap.add_argument("--coarse-box", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--basis", choices=("double", "single"), default="double")
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
    if a.coarse_box > 0:
        out(dict(coarse_box=a.coarse_box, reps=a.reps))
        two_level_section(schwz, torch, a, out)
        return
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
            if a.basis != "double":
                solver.metadata.outer_basis = a.basis
            solver.metadata.max_iters = a.max_iters
            res = solver.solve(None, "zero", gather_solution=False)
            torch.cuda.synchronize()
            added = before - torch.cuda.mem_get_info()[0]
            hist = np.array(res["history"]) / res["rhs_norm"]
            ms = 1e3 * res["elapsed"] / max(res["iter_count"], 1)
            reached = np.nonzero(hist <= rich_rel)[0]
            k_eq = int(reached[0]) if len(reached) else -1
            line = dict(outer="fgmres", basis=a.basis, restart=restart, P=P, iters=res["iter_count"],
                        converged=bool(res["converged"]),
                        cycles=len(res["cycle_starts"]), ms_per_iter=ms, seconds=res["elapsed"],
                        true_rel_residual=res["residual_norm"] / res["rhs_norm"], last_history_rel=float(hist[-1]),
                        iters_to_richardson_residual=k_eq,
                        seconds_to_richardson_residual=(k_eq * ms * 1e-3 if k_eq >= 0 else float("nan")),
                        richardson_seconds=rich["seconds"], richardson_iters=rich["iters"],
                        device_MB_added=added / 2.0 ** 20,
                        vectors_of_n=(2 * restart + 4) if a.basis == "double" else 1.5 * restart + 3.5)
            # where an outer iteration goes: a shorter run that synchronises between the three parts
            solver.outer_profile = True
            solver.metadata.max_iters = min(a.profile_iters, max(res["iter_count"], 1))
            prof = solver.solve(None, "zero", gather_solution=False)
            solver.outer_profile = False
            tot = sum(prof["profile"].values())
            line.update({"share_" + k: v / tot for k, v in prof["profile"].items()})
            line.update(profiled_ms_per_iter=1e3 * tot / max(prof["iter_count"], 1),
                        ortho_seconds=prof["profile"]["ortho"],
                        ortho_ms_per_iter=1e3 * prof["profile"]["ortho"] / max(prof["iter_count"], 1))
            t, nbytes = ortho_rate(schwz, torch, solver._outer["obj"], restart - 1)
            line.update(ortho_ms_at_last_column=1e3 * t, ortho_TBps=nbytes / t * 1e-12)
            out(line)
        solver.metadata.outer_iteration = "richardson"
        del solver
        gc.collect()
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
