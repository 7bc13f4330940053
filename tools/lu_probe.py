"""LU direct local solve: the three measurements behind DESIGN.md "Pivoted LU for the direct local solve".

  1. one device solve y = Q U^-1 L^-1 P b with the LU factors of convdiff 128^2 and 192^2 (RCM pre-order):
     the wave-per-row flag sweep (default dispatch) against the level plan (SCHWZ_TRS_FLAGS=0);
  2. per-step time of the RAS iteration with the LU direct solve against the LL^T one, lap2d 128^2 P = 4
     and ani4_crop x 8;
  3. host schwz_lu against schwz_cholesky on the same matrices.

Run under `rocprofv3 --kernel-trace --stats -- python tools/lu_probe.py` for per-kernel numbers; the
wall-clock figures printed here come from CUDA events / perf_counter.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "schwarz-lib_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import oracle as O  # noqa: E402
import schwz_amd as S  # noqa: E402
from conftest import convection_diffusion_2d  # noqa: E402


def trs_per_solve(f, flags, reps=20):
    if flags is None:
        os.environ.pop("SCHWZ_TRS_FLAGS", None)
    else:
        os.environ["SCHWZ_TRS_FLAGS"] = flags
    t = S.TrsLU(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"], f["row_perm"], f["col_perm"])
    n = len(f["l_rp"]) - 1
    b = torch.tensor(np.random.default_rng(5).standard_normal(n), device="cuda", dtype=torch.float64)
    y = torch.empty_like(b)
    for _ in range(3):
        t.solve(b.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        t.solve(b.data_ptr(), y.data_ptr())
    e1.record()
    torch.cuda.synchronize()
    t.close()
    os.environ.pop("SCHWZ_TRS_FLAGS", None)
    return e0.elapsed_time(e1) / reps, y.cpu().numpy()


def ras_per_step(settings_kw, metadata_kw, P):
    s = S.Settings(**settings_kw)
    m = S.Metadata(num_subdomains=P, **metadata_kw)
    solver = S.SolverRAS(s, m, comm=S.InProcessComm(P), quiet=True)
    t0 = time.perf_counter()
    solver.initialize()
    t1 = time.perf_counter()
    out = solver.run()
    t2 = time.perf_counter()
    solver.close()
    return (t2 - t1) / max(out["iter_count"], 1) * 1e3, out["iter_count"], out["converged"], t1 - t0


def main():
    print("== 1. device solve, LU factors of convdiff (RCM), ms per solve (20 solves, CUDA events)")
    for n in (128, 192):
        rp, col, val = convection_diffusion_2d(n)
        f = S.lu(rp, col, val)
        longest = max(np.diff(f["l_rp"]).max(), np.diff(f["u_rp"]).max())
        tw, yw = trs_per_solve(f, None)
        tl, yl = trs_per_solve(f, "0")
        diff = np.abs(yw - yl).max() / np.abs(yl).max()
        print("convdiff %d^2: n=%d nnz(L)=%d nnz(U)=%d longest row %d | wave sweep %.3f ms | level plan %.3f ms "
              "| ratio %.2f | max rel diff %.1e" % (n, n * n, f["l_rp"][-1], f["u_rp"][-1], longest, tw, tl,
                                                     tl / tw, diff))
    print("== 2. RAS per-step time, direct local solve: LU (umfpack) vs LL^T (cholmod)")
    g = np.load(os.path.join(ROOT, "tests", "golden", "ani4_crop.npz"))
    ani4 = os.path.join("/tmp", "lu_probe_ani4_%d.mtx" % os.getpid())
    rows = np.repeat(np.arange(len(g["rp"]) - 1), np.diff(g["rp"]))
    with open(ani4, "w") as fh:
        fh.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (len(g["rp"]) - 1,
                                                                                  len(g["rp"]) - 1, g["rp"][-1]))
        for r, c, v in zip(rows, g["col"], g["val"]):
            fh.write("%d %d %.17g\n" % (r + 1, c + 1, v))
    cases = [("lap2d 128^2 P=4", dict(), dict(oned_laplacian_size=128, tolerance=1e-8, max_iters=2000), 4),
             ("ani4_crop x 8", dict(matrix_filename=ani4, explicit_laplacian=False),
              dict(tolerance=1e-8, max_iters=3000), 8)]
    for name, skw, mkw, P in cases:
        res = {}
        for fact in ("cholmod", "umfpack"):
            res[fact] = ras_per_step(dict(skw, local_solver="direct-ginkgo", factorization=fact), mkw, P)
        c, u = res["cholmod"], res["umfpack"]
        print("%s: LL^T %.4f ms/step (%d it, conv %s, setup %.2f s) | LU %.4f ms/step (%d it, conv %s, setup "
              "%.2f s) | LU/LL^T %.3f" % (name, c[0], c[1], c[2], c[3], u[0], u[1], u[2], u[3], u[0] / c[0]))
    os.remove(ani4)
    print("== 3. host factorization time (best of 3), whole matrices")
    mats = [("lap2d 128^2", O.laplacian2d(128)), ("ani4_crop", (g["rp"], g["col"], g["val"]))]
    for name, (rp, col, val) in mats:
        tc = min(_timed(S.cholesky, rp, col, val) for _ in range(3))
        tu = min(_timed(S.lu, rp, col, val) for _ in range(3))
        print("%s: schwz_cholesky %.1f ms | schwz_lu %.1f ms | ratio %.2f" % (name, tc, tu, tu / tc))


def _timed(fn, *a):
    t = time.perf_counter()
    fn(*a)
    return (time.perf_counter() - t) * 1e3


if __name__ == "__main__":
    main()
