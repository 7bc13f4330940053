"""The matrices of test_gpu_cg.py, and the child process that solves some of them under switches the library reads
once per process (SCHWZ_CG_QFREE, SCHWZ_CG_SYM, SCHWZ_CG_FUSEDIR, SCHWZ_CG_GRAPH, SCHWZ_SPMV_STREAM,
SCHWZ_STREAM_SEQ, SCHWZ_STREAM_NTY are `static const` there; the parent's process has read them long ago).

  python cg_child.py JOBS.json OUTDIR

JOBS.json: a list of {"case": name, "iters": k, "rtol": r, "env": {...}} (env: switches read per solve, set around
that solve only).  The switches under test are in the environment the parent starts this process with.  Per job
j the iterate goes to OUTDIR/x_j.npy; OUTDIR/result.json lists, per job, the iteration count, the residual norm,
schwz_pcg_flavour and what the upload made of the matrix.  Not a test module: pytest does not collect it; the
parent owns the references and every assertion."""
import json
import os
import sys

import numpy as np

GRAPH_ROWS = 1 << 21      # kGraphRows of schwz_internal.hpp

# switches read when a matrix is uploaded
PAIRS = {"SCHWZ_SPMV_PATTERN": "2", "SCHWZ_SPMV_PAIR": "2"}
PLAIN = {"SCHWZ_SPMV_PATTERN": "0", "SCHWZ_SPMV_PAIR": "0", "SCHWZ_SPMV_DICT": "0"}
DICT = {"SCHWZ_SPMV_PATTERN": "0", "SCHWZ_SPMV_PAIR": "0", "SCHWZ_SPMV_DICT": "2"}
SMALL_WALK = dict(PAIRS, SCHWZ_SPMV_SWEEP="2", SCHWZ_SWEEP_T="512", SCHWZ_SWEEP_L="4")

# name -> (grid shape, switches at upload).  Every matrix is the Dirichlet Laplacian of its grid (Jacobi: a uniform
# diagonal), so hp.stencil_apply is its reference operator.
#   cube128      2^21 rows exactly: the last size that replays graphs and updates x in the loop
#   past128      the first size past it: deferred x, every launch in the z-sweep walk
#   lines3       three x lines per plane: row pairs, symmetric, but no canonical layout -- no walk (2 150 400 rows)
#   lines3_full  the same without the upper-triangle tables (p.(A p) from full rows: kSpmvDotOnly)
#   lines3_csr / lines3_dict  the same in plain CSR / per-entry dictionaries: the stored-q iteration
#   walk_small / walk_small8 / pair_small / csr_small  12 288 / 24 576 / 8 160 rows: the walk forced on small
#                grids (planes of 1024 and 2048 rows), row pairs, plain CSR
#   gen520       520 x 520: planes (x lines) that are no multiple of 512 rows -- the walk's "gen mode", forced small
GRIDS = {
    "cube128": ((128, 128, 128), {}),
    "past128": ((128, 128, 129), {}),
    "lines3": ((1024, 3, 700), {}),
    "lines3_full": ((1024, 3, 700), {"SCHWZ_SPMV_SYM": "0"}),
    "lines3_csr": ((1024, 3, 700), PLAIN),
    "lines3_dict": ((1024, 3, 700), DICT),
    "walk_small": ((256, 4, 12), SMALL_WALK),
    "walk_small8": ((256, 8, 12), SMALL_WALK),
    "pair_small": ((24, 20, 17), PAIRS),
    "csr_small": ((24, 20, 17), PLAIN),
    "gen520": ((520, 520), dict(PAIRS, SCHWZ_SPMV_SWEEP="2")),
}


def paths():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "schwarz-lib_amd"), os.path.join(root, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)


def laplacian(oracle, shape):
    if len(shape) == 3:
        rp, col, val = oracle.laplacian3d(*shape)
    else:
        assert shape[0] == shape[1]
        rp, col, val = oracle.laplacian2d(shape[0])
    return np.asarray(rp, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64)


def variable_coefficients(shape, levels, seed):
    """Symmetric 7-point matrix with one coefficient per grid edge: -c_e off the diagonal, the sum of a row's six
    coefficients (edges through the boundary count 1) on it -- irreducibly diagonally dominant, hence SPD.
    levels = 0: coefficients uniform in [0.5, 1.5) (as many diagonal values as rows); levels = k: coefficients from
    {1, ..., k} (at most 5 k + 1 diagonal values: the Jacobi diagonal fits a dictionary for k = 2)."""
    import scipy.sparse as sp
    nx, ny, nz = shape
    n = nx * ny * nz
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    coord = (i % nx, (i // nx) % ny, i // (nx * ny))
    diag = np.zeros(n)
    rows, cols, vals = [], [], []
    for ax, off in enumerate((1, nx, nx * ny)):
        has = coord[ax] < shape[ax] - 1                      # the edge (i, i + off) exists
        c = rng.uniform(0.5, 1.5, n) if levels == 0 else rng.integers(1, levels + 1, n).astype(np.float64)
        c = np.where(has, c, 1.0)                            # towards the upper boundary
        diag += c
        diag[off:] += np.where(has[:-off], c[:-off], 0.0)    # the same edge seen from its other end
        diag += np.where(coord[ax] == 0, 1.0, 0.0)           # towards the lower boundary
        rows += [i[has], i[has] + off]
        cols += [i[has] + off, i[has]]
        vals += [-c[has], -c[has]]
    rows.append(i), cols.append(i), vals.append(diag)
    a = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def rhs(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), 0.1 * rng.standard_normal(n)


class upload_env:
    """The switches read at upload / per solve, set for the duration of a `with` block."""

    def __init__(self, env):
        self.env = dict(env)

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def describe(A):
    return dict(format=A.format(), symmetric=A.symmetric(), slots=A.sweep_slots(), left_out=A.sweep_left_out())


def main(argv):
    jobs = json.load(open(argv[1]))
    out = argv[2]
    paths()
    import torch
    import oracle
    import schwz_amd as schwz
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    oracle.build()
    held = {}
    results = []
    for j, job in enumerate(jobs):
        name = job["case"]
        if name not in held:
            held.clear()   # one matrix at a time in HBM
            shape, env = GRIDS[name]
            rp, col, val = laplacian(oracle, shape)
            with upload_env(env):
                A = schwz.Csr(rp, col, val)
                held[name] = (A, schwz.Pcg(A, 1), len(rp) - 1)
            del rp, col, val
        A, cg, n = held[name]
        b, x0 = rhs(n, job.get("seed", 1))
        d_b = torch.from_numpy(b).cuda()
        d_x = torch.from_numpy(x0).cuda()
        with upload_env(job.get("env", {})):
            it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), float(job["rtol"]), int(job["iters"]))
        np.save(os.path.join(out, "x_%d.npy" % j), d_x.cpu().numpy())
        results.append(dict(describe(A), case=name, n=n, iters=it, resnorm=rn, flavour=cg.flavour()))
    with open(os.path.join(out, "result.json"), "w") as f:
        json.dump(results, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
