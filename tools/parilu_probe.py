"""ParILU factors and Jacobi-sweep triangular solves against the exact ILU(0) path: the measurements behind
DESIGN.md "ParILU and Jacobi-sweep triangular solves" (profiles/r05_parilu_probe.txt).

  python tools/parilu_probe.py cg <edge> <precond: ilu | isai | jacobi> <par_ilu_sweeps> <trisolve_sweeps>
  python tools/parilu_probe.py gmres <edge> <precond> <par_ilu_sweeps> <trisolve_sweeps>

cg: 3-D Poisson edge^3 (P = 1, the local matrix of bench.py's subdomain), CG to rtol 1e-10 from x = 0.
gmres: convdiff edge^2, GMRES(30) to rtol 1e-10.  One line per run: preconditioner setup seconds (with
SCHWZ_SETUP_TIMING=1 the library prints its stages on stderr), iterations, ms per iteration, time to
solution.  Run under `rocprofv3 --kernel-trace --stats -- python tools/parilu_probe.py ...` for per-kernel
numbers.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "schwarz-lib_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import schwz_amd as S  # noqa: E402
from conftest import convection_diffusion_2d  # noqa: E402

PRECONDS = {"ilu": S.capi.PRECOND_ILU, "isai": S.capi.PRECOND_ISAI, "jacobi": S.capi.PRECOND_JACOBI}


def main():
    kind, edge, name = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    par, tri = int(sys.argv[4]), int(sys.argv[5])
    if kind == "cg":
        prob = S.Problem.laplacian(3, edge, edge, edge)
        sd = S.Subdomain(prob, 1, 0, 2, S.partition_regular(prob.N, 1))
        rp, col, val = sd.local_matrix()
        label = "lap3d %d^3" % edge
    else:
        rp, col, val = convection_diffusion_2d(edge)
        label = "convdiff %d^2" % edge
    n = len(rp) - 1
    A = S.Csr(rp, col, val)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if kind == "cg":
        solver = S.Pcg(A, PRECONDS[name], par_ilu_sweeps=par, trisolve_sweeps=tri)
    else:
        solver = S.Gmres(A, PRECONDS[name], restart=30, par_ilu_sweeps=par, trisolve_sweeps=tri)
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    solver.solve(b.data_ptr(), x.data_ptr(), 0.0, 20)   # warm-up (records the graphs of the CG loop, if any)
    torch.cuda.synchronize()
    x.zero_()
    maxit = 20000
    t0 = time.perf_counter()
    it, rn = solver.solve(b.data_ptr(), x.data_ptr(), 1e-10, maxit)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    import scipy.sparse as sp
    M = sp.csr_matrix((val, col, rp), shape=(n, n))
    true_rel = np.linalg.norm(1.0 - M @ x.cpu().numpy()) / np.sqrt(n)
    print("RESULT %s %s par_ilu_sweeps=%d trisolve_sweeps=%d setup %.3f s iterations %d ms/iteration %.3f "
          "solve %.3f s true_rel_res %.2e" % (label, name, par, tri, setup, it, 1e3 * el / max(it, 1), el, true_rel),
          flush=True)


if __name__ == "__main__":
    main()
