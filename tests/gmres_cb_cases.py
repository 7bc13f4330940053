"""The cases of tests/test_gpu_gmres_basis.py and their references, computed once per process and shared (not a test
module: pytest does not collect it).  A case is (matrix, size, restart m, preconditioner code, rtol, max_iters); its
references are the restatement of hp_gmres_cb.py in np.longdouble and, the same text, in float64.

Sizes.  A lane of the pass kernels holds four consecutive rows (one 16-byte load of an fp32 column), a workgroup 1024
rows, and the grid is capped at 1024 workgroups: 1 and 3 rows are below one 16-byte load; 255, 256, 257 end inside,
at the end of and one past a 16-byte load of the 64th lane; 1023, 1024, 1025 do the same at the end of the first
workgroup; 524 289 is one row past kBlock * kMaxGrid lanes; 1 048 577 is one row past 1024 workgroups of 1024 rows:
the pass kernels stride, and the one lane that makes a second trip finds a single row there.
Restart lengths: 1, 8 (a full group of basis columns), 9 (one past a group), 30 (four groups, the last of six).
max_iters 70 and 100 are no multiples of 8, 9 or 30.
"""
import numpy as np

import hp_gmres_cb
import hp_reference as hp
from conftest import convection_diffusion_2d

LD = hp.LD

# |iterations(float64 restatement) - iterations(longdouble restatement)|, the largest over CASES: measured by
# test_gmres_basis_options.py::test_iteration_spread_of_the_restatements, which fails if a case exceeds it
# (profiles/r23_gmres_basis.txt records the figure).  The device count may differ from the longdouble count by one
# more than this.
SPREAD = 0


def tridiag(n, lo=-1.3, d=2.5, up=-0.7):
    import scipy.sparse as sp
    a = sp.diags([np.full(max(n - 1, 0), lo), np.full(n, d), np.full(max(n - 1, 0), up)], [-1, 0, 1], shape=(n, n),
                 format="csr")
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def matrix(kind, size):
    return tridiag(size) if kind == "tri" else convection_diffusion_2d(size)


SMALL = [("tri", n, m, 0, 1e-8, 70) for n in (1, 3, 255, 256, 257, 1023, 1024, 1025) for m in (1, 8, 9, 30)] + \
        [("cd", k, m, 1, 1e-8, 100) for k in (3, 16, 17, 33) for m in (1, 8, 9, 30)]
# fixed work (rtol = 0) where the longdouble restatement costs seconds per iteration
LARGE = [("tri", 524289, 9, 0, 0.0, 11), ("tri", 1048577, 2, 0, 0.0, 3)]
CASES = SMALL + LARGE


def case_id(case):
    kind, size, m, pc, rtol, maxit = case
    return "%s%d-m%d" % (kind, size, m)


def rhs(n, seed=29):
    rng = np.random.default_rng(seed + n)
    return rng.standard_normal(n), rng.standard_normal(n) * 0.1


class Ref:
    """Both restatements of one case and what the checks take from them."""

    def __init__(self, case):
        kind, size, m, pc, rtol, maxit = case
        self.case = case
        self.rp, self.col, self.val = matrix(kind, size)
        self.n = len(self.rp) - 1
        self.b, self.x0 = rhs(self.n)
        self.hist, self.x, self.cycles = {}, {}, {}
        for dt in (LD, np.float64):
            M = hp.precond_jacobi(self.rp, self.col, self.val, dt) if pc == 1 else hp.precond_none(dt)
            cyc = []
            x, h = hp_gmres_cb.gmres_cb(self.rp, self.col, self.val, self.b, self.x0, M, maxit, m, rtol, dt,
                                        cycle_starts=cyc)
            self.x[dt], self.hist[dt], self.cycles[dt] = x, h, cyc
        h = self.hist[LD]
        self.iters = len(h) - 1
        self.iters64 = len(self.hist[np.float64]) - 1
        self.r0 = float(h[0])
        self.recurred = float(h[-1] / h[0])                       # what the stop test saw, relative
        self.true = hp_gmres_cb.true_relres(self.rp, self.col, self.val, self.x[LD], self.b, self.x0)
        # the restatement's own ratio of true to recurred residual, doubled; two is the floor
        self.factor = max(2.0, 2.0 * self.true / self.recurred) if self.recurred > 0 else 2.0
        # the residual the solve was stopped at: the tolerance, or what max_iters left
        self.target = max(rtol, self.recurred)
        self.beta_last = float(self.cycles[LD][-1][1]) if self.cycles[LD] else 0.0


_refs = {}


def ref(case):
    if case not in _refs:
        hp.require_extended_precision()
        _refs[case] = Ref(case)
    return _refs[case]
