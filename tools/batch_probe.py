"""What a block of right-hand sides costs against one right-hand side after the other (csrc/batch.hip).

Part 1, the local solver alone: time per inner iteration of BatchCg (Jacobi) for K = 2, 4, 8 against the single-vector
CG on plain CSR (the matrix uploaded with the codings off: what spmv_variant = 6 runs) and against the default
single-vector path (the coding the upload chooses: on a 3-D Laplacian the z-sweep walk), on

  lap256     the 256^3 Laplacian, 16.8 M rows
  ani4x512   tests/golden/ani4_crop replicated 512 times block-diagonally, 1.6 M rows: a general matrix
  ani4x8     the same 8 times, 24648 rows: a launch-bound size

Every solver runs fixed-work solves (rtol = 0) of `--iters` and of twice as many iterations between two device events,
nothing read back; the time per iteration is the difference of the two medians over the difference of the counts, i.e.
without the start launches.  The solvers alternate inside every round.  Per column: that time over K.  Bytes: the model
of the README per iteration, 12 nnz + 4 (n + 1) matrix bytes once and 100 n vector bytes per column -- a model, the
ratio to it is printed as "model TB/s".

Part 2, the outer iteration: SolverRAS.solve_many of 4 and of 8 columns against as many solve() calls on the same
solver, on 1 and on 4 in-process subdomains, Jacobi, 10 fixed inner iterations, tolerance 1e-6: the `elapsed` of the
runs (the loops, between device synchronisations), alternating, and the outer iteration counts.

  python tools/batch_probe.py [--problems lap256,ani4x512,ani4x8] [--outer lap128,lap29] [--rounds 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "schwarz-lib_amd"), os.path.join(ROOT, "tools")]
CODINGS = ("SCHWZ_SPMV_PAIR", "SCHWZ_SPMV_PATTERN", "SCHWZ_SPMV_DICT")


def host_matrix(schwz, problem):
    if problem.startswith("lap"):
        n = int(problem[3:])
        rp, col, val = schwz.Problem.laplacian(3, n, n, n).to_csr()
        return np.asarray(rp), np.asarray(col), np.asarray(val)
    from cheb_probe import ani4_replicated
    return ani4_replicated(int(problem[5:]))


def upload(schwz, csr, codings):
    saved = {k: os.environ.get(k) for k in CODINGS}
    if not codings:
        os.environ.update({k: "0" for k in CODINGS})   # read at the upload
    try:
        return schwz.Csr(*csr)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def timed_solve(torch, solver, d_b, d_x, x0, iters):
    d_x.copy_(x0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    solver.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, iters, want_stats=False)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def part_one(schwz, torch, say, problem, iters, rounds):
    csr = host_matrix(schwz, problem)
    n, nnz = len(csr[0]) - 1, int(csr[0][-1])
    A_plain, A_default = upload(schwz, csr, False), upload(schwz, csr, True)
    del csr
    say("%s: %d rows, %d nonzeros (%.1f per row); default coding: format %d" % (problem, n, nnz, nnz / n, A_default.format()))
    rng = np.random.default_rng(5)
    solvers = [("cg plain CSR", 1, schwz.Pcg(A_plain, schwz.capi.PRECOND_JACOBI)),
               ("cg default", 1, schwz.Pcg(A_default, schwz.capi.PRECOND_JACOBI))]
    solvers += [("block K=%d" % K, K, schwz.BatchCg(A_plain, schwz.capi.PRECOND_JACOBI, K)) for K in (2, 4, 8)]
    bufs = {}
    for K in (1, 2, 4, 8):
        b = torch.from_numpy(rng.standard_normal(n * K)).cuda()
        x0 = torch.from_numpy(rng.standard_normal(n * K) * 0.1).cuda()
        bufs[K] = (b, torch.empty_like(x0), x0)
    times = {(name, m): [] for name, _, _ in solvers for m in (1, 2)}
    for name, K, s in solvers:      # warm-up: code objects, graphs, first-use allocations
        for m in (1, 2):
            timed_solve(torch, s, *bufs[K], m * iters)
    for _ in range(rounds):
        for name, K, s in solvers:
            for m in (1, 2):
                times[(name, m)].append(timed_solve(torch, s, *bufs[K], m * iters))
    per = {}
    for name, K, _ in solvers:
        med = {m: statistics.median(times[(name, m)]) for m in (1, 2)}
        per[name] = (med[2] - med[1]) / iters * 1e3 / K          # us per column and iteration
        model = 12 * nnz + 4 * (n + 1) + 100 * n * K
        say("  %-13s %3d / %3d iterations: %9.3f / %9.3f ms (min %.3f / %.3f); us per iteration %9.2f, per column %9.2f; "
            "model %.0f B per column and row, %.2f model TB/s"
            % (name, iters, 2 * iters, med[1], med[2], min(times[(name, 1)]), min(times[(name, 2)]), per[name] * K, per[name],
               model / n / K, model / (per[name] * K * 1e-6) / 1e12))
    for name, K, _ in solvers[2:]:
        say("  %-13s per column and iteration: %.3f x the plain-CSR CG, %.3f x the default CG (below 1: the block wins)"
            % (name, per[name] / per["cg plain CSR"], per[name] / per["cg default"]))
    del solvers, bufs, A_plain, A_default
    torch.cuda.empty_cache()


def part_two(schwz, torch, say, problem, P, rounds):
    n = int(problem[3:])
    N = n ** 3
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(n, n, n), overlap=2)
    m = schwz.Metadata(num_subdomains=P, tolerance=1e-6, max_iters=400, local_precond="block-jacobi",
                       precond_max_block_size=1, local_solver_tolerance=0.0, local_max_iters=10)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    B = np.random.default_rng(9).standard_normal((N, 8))
    for ncol in (4, 8):
        single, many, its_s, its_m = [], [], None, None
        for r in range(rounds + 1):        # round 0 warms up
            t = 0.0
            outs = []
            for j in range(ncol):
                out = solver.solve(B[:, j], gather_solution=False)
                t += out["elapsed"]
                outs.append(out["iter_count"])
            out = solver.solve_many(B[:, :ncol], gather_solution=False)
            if r:
                single.append(t)
                many.append(out["elapsed"])
            its_s, its_m = outs, out["iter_count"]
        say("  %s, %d subdomain(s), %d columns: %d solve() calls %.2f ms (min %.2f), solve_many %.2f ms (min %.2f): "
            "%.3f x; outer iterations %s against %s"
            % (problem, P, ncol, ncol, statistics.median(single) * 1e3, min(single) * 1e3, statistics.median(many) * 1e3,
               min(many) * 1e3, statistics.median(many) / statistics.median(single), its_s, its_m))
    del solver
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="lap256,ani4x512,ani4x8")
    ap.add_argument("--outer", default="lap128,lap29")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import schwz_amd as schwz
    if not torch.cuda.is_available():
        sys.exit("batch_probe: no GPU (nothing here can be measured on a CPU)")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("batch_probe on %s: %d and %d inner iterations, %d alternating rounds" %
        (torch.cuda.get_device_name(0), a.iters, 2 * a.iters, a.rounds))
    for problem in [p for p in a.problems.split(",") if p]:
        part_one(schwz, torch, say, problem, a.iters, a.rounds)
    say("solve_many against repeated solve(): Jacobi, 10 fixed inner iterations, tolerance 1e-6")
    for problem in [p for p in a.outer.split(",") if p]:
        for P in (1, 4):
            part_two(schwz, torch, say, problem, P, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
