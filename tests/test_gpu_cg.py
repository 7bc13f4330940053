"""Device-resident CG (csrc/cg.hip and the SpMV launches it drives) against the extended-precision restatement
hp.pcg, at the sizes the library changes its plan at: both sides of kGraphRows = 2^21 rows, the benchmark's 256^3
cube and the z-slabs of its multi-GPU runs, the q-free iteration with and without the z-sweep walk, the stored-q
iteration with the deferred x update, the general preconditioners past the launch cap, the edges of the vector
kernels, stops on a tolerance, the postponed tail of a fixed-work solve, and (in child processes, cg_child.py)
the switches the library reads once per process.

Tolerance.  As in test_gpu_gmres.py there is no useful a-priori bound for CG iterates, so every case computes the
reference twice from one text, in longdouble and in float64, and takes dev = |x_f64 - x_ld|_inf / |x_ld|_inf (and
the same for the recurred residual norm) as the size of legitimate float64 rounding.  The device must stay within
MARGIN * max(dev, iters * 2^-52) of the longdouble result.  MARGIN = 32 for the reason given there: the kernels fold
r.z, p.(A p) and ||r||^2 from up to 2048 per-workgroup partial sums in an order numpy's pairwise sum does not
use.  The reference sizes the tolerance; the kernel's output never does.  tools/hp_reference_probe.py prints the
measured ratios (profiles/r08_cg_reference.txt).

Every case asserts the flavour (schwz_pcg_flavour) that pcg_plan_matrix / pcg_plan_solve / pcg_plan_flavour give
for it -- plan_flavour() below restates them -- so that no case passes on another path than the one it names.
The benchmark's three flavours: 254 (cube, slabs, past128), 18 (cube128, and past128 with graphs forced), 4
(plain-CSR and dictionary codings past 2^21 rows).

Skips: no extended precision; too little free HBM for the 256^3 cube and the slabs; the child-process cases after a
child died on a signal or a timeout (nothing more is started on the card)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import cg_child as cc
import hp_reference as hp

pytestmark = pytest.mark.gpu

LD = np.longdouble
MARGIN = 32.0
# (case, rows, iters, flavour, dev x, floor, x err / dev, dev resn, resn err / dev, unfloored dev x)
RATIOS = []
# (case, stop iteration, rtol, reduction at the stop / rtol, smallest earlier reduction / rtol)
SEPARATION = []
NOTES = []            # free HBM seen by the large cases, wall times
D0, D2 = {"SCHWZ_CG_DEFERX": "0"}, {"SCHWZ_CG_DEFERX": "2"}   # read per solve
SMALL_COUNTS = (5, 16, 17, 31, 33)
BIG_HBM = 24 << 30    # the cube: 1.9 GB of matrix and codings, 0.5 GB of vectors; a slab the same -- a wide margin


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _inf(a):
    return float(np.abs(a).max()) if len(a) else 0.0


# ---- the plan, restated ------------------------------------------------------------------------------------------

def plan_flavour(n, fmt, sym, walk, covers, rtol, iters, env=None, general=False, diag="uniform"):
    """schwz_pcg_flavour as pcg_plan_matrix, pcg_plan_solve and pcg_plan_flavour (csrc/cg.hip) derive it.
    fmt / sym / walk / covers: Csr.format(), .symmetric(), .sweep_slots() > 0, .sweep_left_out() == 0 (the walk
    serves every row: a solve may start in it); diag: how the Jacobi diagonal travels ("none", "uniform",
    "vector", "dict"); env: the switches in force (over the process environment)."""
    env = dict(env or {})

    def get(k, d):
        return env.get(k, os.environ.get(k, d))

    def on(k):
        return get(k, "1")[:1] != "0"
    qfree = on("SCHWZ_CG_QFREE") and not general and fmt == 3 and diag != "dict"
    dot_sym = qfree and on("SCHWZ_CG_SYM") and sym
    sweep_on = on("SCHWZ_CG_SWEEP") and walk and diag != "dict"
    sweep_dirdot = sweep_on and sym and diag != "vector"
    fm = int(get("SCHWZ_CG_FUSEDIR", "1"))
    fusedir = dot_sym and (fm == 2 or (fm == 1 and (n <= cc.GRAPH_ROWS or sweep_dirdot)))
    dm = int(get("SCHWZ_CG_DEFERX", "1"))
    deferx = not general and (dm == 2 or (dm == 1 and n > cc.GRAPH_ROWS))
    start = on("SCHWZ_CG_SWEEPSTART") and deferx and sweep_dirdot and fusedir and covers
    all_walks = fusedir and start and qfree and diag in ("none", "uniform")
    p0_virtual = on("SCHWZ_CG_P0VIRTUAL") and start and all_walks and iters >= 2
    lazy = on("SCHWZ_CG_LAZYLAST") and rtol == 0.0 and deferx and iters > 0
    vlast = lazy and on("SCHWZ_CG_PLASTVIRTUAL") and iters >= 2 and all_walks
    return ((0 if not qfree else 2 if fusedir else 1) | (4 if deferx else 0) | (8 if sweep_on and deferx else 0) |
            (16 if sweep_dirdot and fusedir else 0) | (32 if start else 0) | (64 if p0_virtual else 0) |
            (128 if vlast else 0))


def test_plan_restatement_gives_the_flavours_the_benchmark_records():
    big = cc.GRAPH_ROWS + 1
    assert plan_flavour(big, 3, True, True, True, 0.0, 10) == 254
    assert plan_flavour(big, 3, True, True, True, 1e-3, 10) == 126
    assert plan_flavour(big, 3, True, True, True, 0.0, 1) == 62
    assert plan_flavour(cc.GRAPH_ROWS, 3, True, True, True, 0.0, 10) == 18
    assert plan_flavour(big, 0, False, False, True, 0.0, 10) == 4
    assert plan_flavour(big, 3, True, False, True, 0.0, 10) == 5
    assert plan_flavour(big, 3, False, False, True, 0.0, 10) == 5
    assert plan_flavour(big, 0, False, False, True, 0.0, 10, general=True) == 0


# ---- comparison --------------------------------------------------------------------------------------------------

def compare(tag, n, flavour, iters, got, rn, x_ld, r_ld, x_64, r_64, check_resn=True):
    floor = max(iters, 1) * 2.0 ** -52
    scale = _inf(x_ld)
    raw_x = _inf(x_64 - x_ld) / scale          # float64 - longdouble: numpy computes in longdouble
    dev_x = max(raw_x, floor)
    err_x = _inf(got - x_ld) / scale
    r_ld, r_64 = float(r_ld), float(r_64)
    dev_r = max(abs(r_64 - r_ld) / r_ld, floor) if r_ld > 0 else floor
    err_r = abs(rn - r_ld) / r_ld if r_ld > 0 else abs(rn)
    RATIOS.append((tag, n, iters, flavour, dev_x, floor, err_x / dev_x, dev_r, err_r / dev_r if check_resn else -1.0, raw_x))
    print("%s iters %d flavour %d: x err %.2e = %.2f dev (dev %.2e), resn err %.2e = %.2f dev" %
          (tag, iters, flavour, err_x, err_x / dev_x, dev_x, err_r, err_r / dev_r))
    assert np.isfinite(got).all() and np.isfinite(rn)
    assert err_x <= MARGIN * dev_x, (tag, iters, err_x, dev_x)
    if check_resn:
        assert err_r <= MARGIN * dev_r, (tag, iters, err_r, dev_r)


class Case:
    """One matrix on the device and both references on the host.  op / M: dtype -> (v -> A v) / (v -> M^-1 v)."""

    def __init__(self, schwz, torch, tag, rp, col, val, op, M, precond=1, bs=1, env=None, diag="uniform"):
        self.schwz, self.torch, self.tag = schwz, torch, tag
        self.n = len(rp) - 1
        self.op, self.M, self.diag = op, M, ("none" if precond == 0 else diag)
        self.general = precond >= 2
        with cc.upload_env(env or {}):
            self.A = schwz.Csr(rp, col, val)
            self.cg = schwz.Pcg(self.A, precond, bs)
        self.refs = {}

    @property
    def info(self):
        return cc.describe(self.A)

    def expect(self, rtol, iters, env=None):
        d = self.info
        return plan_flavour(self.n, d["format"], d["symmetric"], d["slots"] > 0, d["left_out"] == 0, rtol, iters, env,
                            self.general, self.diag)

    def reference(self, b, x0, counts, key=0):
        """{dtype: (x after c updates for c in counts, history)}, computed once per (key, counts)."""
        k = (key, tuple(counts))
        if k not in self.refs:
            out = {}
            for dt in (LD, np.float64):
                keep = {c: None for c in counts}
                _, hist = hp.pcg(self.op(dt), None, None, b, x0, self.M(dt), max(counts), dtype=dt, keep=keep)
                out[dt] = (keep, hist)
            self.refs[k] = out
        return self.refs[k]

    def device(self, b, x0, rtol, iters, env=None, want_stats=True):
        d_b = _dev(self.torch, b)
        d_x = _dev(self.torch, x0 if x0 is not None else np.zeros(self.n))
        with cc.upload_env(env or {}):
            it, rn = self.cg.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, iters, want_stats=want_stats)
        return d_x.cpu().numpy(), it, rn, self.cg.flavour()

    def check_fixed(self, b, x0, counts, key=0, env=None, flavour=None, check_resn=True, ref_counts=None):
        """`counts` fixed-work solves (rtol = 0) against the reference run (which keeps ref_counts, default counts)."""
        ref = self.reference(b, x0, ref_counts or counts, key)
        assert len(ref[LD][1]) - 1 == len(ref[np.float64][1]) - 1 == max(ref_counts or counts)
        for c in counts:
            got, it, rn, fl = self.device(b, x0, 0.0, c, env)
            want = self.expect(0.0, c, env)
            assert fl == want, (self.tag, c, fl, want)
            if flavour is not None:
                assert fl == (flavour(c) if callable(flavour) else flavour), (self.tag, c, fl)
            assert it == c, (self.tag, it, c)
            compare(self.tag, self.n, fl, c, got, rn, ref[LD][0][c], ref[LD][1][c], ref[np.float64][0][c],
                    ref[np.float64][1][c], check_resn)

    def check_stop(self, b, x0, target, counts, key=0, env=None, flavour=None):
        """A stop on a tolerance at update `target`: rtol from the longdouble history alone, separated from the
        reductions on either side of it by more than 1e-6, in both reference runs; then the device must stop at
        exactly that update."""
        assert target in counts
        ref = self.reference(b, x0, counts, key)
        rtol = None
        for dt in (LD, np.float64):
            h = np.array([float(v) for v in ref[dt][1]])
            before = h[:target].min()
            if rtol is None:
                assert h[target] < before, "update %d is no new minimum of the reference's history" % target
                rtol = float(np.sqrt(h[target] * before) / h[0])
                SEPARATION.append((self.tag, target, rtol, h[target] / h[0] / rtol, before / h[0] / rtol))
            assert h[target] <= (1 - 1e-6) * rtol * h[0] and before >= (1 + 1e-6) * rtol * h[0], (self.tag, dt, target)
        got, it, rn, fl = self.device(b, x0, rtol, max(4 * target, 64), env)
        want = self.expect(rtol, max(4 * target, 64), env)
        assert fl == want and fl & 128 == 0, (self.tag, fl, want)
        if flavour is not None:
            assert fl == flavour, (self.tag, fl)
        assert it == target, (self.tag, it, target)
        compare(self.tag + ("/stop+ring" if env else "/stop"), self.n, fl, target, got, rn, ref[LD][0][target], ref[LD][1][target],
                ref[np.float64][0][target], ref[np.float64][1][target])
        return rtol


def _grid_case(schwz, oracle, torch, name, precond=1):
    """A Case for one of cg_child.GRIDS: the slicing stencil is its operator, Jacobi divides by 2 * dim."""
    shape, env = cc.GRIDS[name]
    rp, col, val = cc.laplacian(oracle, shape)

    def op(dt):
        return lambda v: hp.stencil_apply(v, shape, dt)

    def M(dt):
        d = np.dtype(dt).type(2 * len(shape))
        return (lambda v: v / d) if precond == 1 else hp.precond_none(dt)
    return Case(schwz, torch, name if precond == 1 else name + "/none", rp, col, val, op, M, precond, env=env)


_CASES = {}


def grid_case(schwz, oracle, torch, name):
    """Cases that several tests share (their references are computed once); two matrices of 2 M rows are cheap to
    hold, the 17 M row ones are built and dropped by their own test."""
    if name not in _CASES:
        _CASES[name] = _grid_case(schwz, oracle, torch, name)
    return _CASES[name]


def _need_hbm(torch):
    hp.require_extended_precision()
    free = torch.cuda.mem_get_info()[0]
    NOTES.append("free HBM seen: %.1f GiB" % (free / 2.0 ** 30))
    if free < BIG_HBM:
        pytest.skip("%.1f GiB of free HBM: too little for the 17 M row cases" % (free / 2.0 ** 30))


# ---- the default plan above 2^21 rows, no CG switch forced ---------------------------------------------------------

def _last_new_minimum(h, upto):
    h = np.array([float(v) for v in h])
    return max(t for t in range(2, upto + 1) if h[t] < (1 - 1e-3) * h[:t].min())


def test_cg_on_the_256_cube_the_benchmarks_operating_point(schwz, oracle, torch_cuda):
    """256^3 = 16.7 M rows, Jacobi, rtol = 0, 10 updates: what bench.py times (flavour 254), and a stop on a
    tolerance on the same matrix (lazy last and virtual last direction off: 126)."""
    _need_hbm(torch_cuda)
    shape = (256, 256, 256)
    rp, col, val = cc.laplacian(oracle, shape)
    c = Case(schwz, torch_cuda, "cube256", rp, col, val, lambda dt: (lambda v: hp.stencil_apply(v, shape, dt)),
             lambda dt: (lambda v: v / np.dtype(dt).type(6)))
    del rp, col, val
    d = c.info
    assert d["format"] == 3 and d["symmetric"] and d["slots"] > 0 and d["left_out"] == 0, d
    b, x0 = cc.rhs(c.n, 1)
    counts = tuple(range(2, 11))
    ref = c.reference(b, x0, counts)
    c.check_fixed(b, x0, (10,), flavour=254, ref_counts=counts)
    target = _last_new_minimum(ref[LD][1], 9)
    c.check_stop(b, x0, target, counts, flavour=126)


@pytest.mark.parametrize("me", [1, 2])
def test_cg_on_the_slabs_of_512_x_512_x_192_in_three(schwz, torch_cuda, me):
    """The local_matrix() of a middle and an end z-slab (17 M rows: 64 planes and one overlap plane per neighbour,
    appended behind the interior and chained into the walk).  The reference applies the slicing stencil to the
    slab's box in natural order, permuted with the subdomain's own index set (pinned against local_matrix on the
    CPU, test_hp_reference.py)."""
    _need_hbm(torch_cuda)
    nx, ny, nz = 512, 512, 192
    prob = schwz.Problem.laplacian(3, nx, ny, nz)
    sd = schwz.Subdomain(prob, 3, me, 2, schwz.partition_regular(prob.N, 3))
    rp, col, val = sd.local_matrix()
    l2g = sd.local_to_global[:len(rp) - 1].copy()
    del sd, prob
    c = Case(schwz, torch_cuda, "slab%d" % me, rp, col, val, lambda dt: hp.slab_operator(l2g, nx, ny, dt),
             lambda dt: (lambda v: v / np.dtype(dt).type(6)))
    del rp, col, val
    assert c.n == (nz // 3 + (2 if me == 1 else 1)) * nx * ny
    d = c.info
    assert d["format"] == 3 and d["symmetric"] and d["slots"] > 0 and d["left_out"] == 0, d
    b, x0 = cc.rhs(c.n, 2 + me)
    c.check_fixed(b, x0, (10,), flavour=254)


def test_cg_on_a_2d_grid_of_1500_squared(schwz, oracle, torch_cuda):
    """2.25 M rows of the 5-point stencil: x lines of 1500 rows in the role of the planes (no multiple of 512: the
    walk's gen mode), the whole solve in the walk."""
    hp.require_extended_precision()
    shape = (1500, 1500)
    rp, col, val = cc.laplacian(oracle, shape)
    c = Case(schwz, torch_cuda, "grid1500", rp, col, val, lambda dt: (lambda v: hp.stencil_apply(v, shape, dt)),
             lambda dt: (lambda v: v / np.dtype(dt).type(4)))
    d = c.info
    assert d["format"] == 3 and d["symmetric"] and d["slots"] > 0 and d["left_out"] == 0, d
    b, x0 = cc.rhs(c.n, 5)
    c.check_fixed(b, x0, (1, 10, 19), flavour=lambda k: 62 if k == 1 else 254)


# ---- both sides of kGraphRows ----------------------------------------------------------------------------------------

RING_COUNTS = (1, 2, 15, 16, 17, 33, 48)


@pytest.mark.parametrize("name", ["cube128", "past128"])
def test_cg_on_both_sides_of_the_graph_threshold(schwz, oracle, torch_cuda, name):
    """128^3 = 2^21 rows: graphs of 16 iterations, x updated in the loop, the fused launch in the walk (18).
    128 x 128 x 129: no graphs, x deferred into the ring of 16, every launch in the walk, virtual first and last
    direction (254; one update: 62).  15, 16, 17, 33, 48 updates: below, at and past one replay / one ring, two
    and a partial third, three exactly; 1 and 2: p0_virtual and vlast need two."""
    hp.require_extended_precision()
    c = grid_case(schwz, oracle, torch_cuda, name)
    d = c.info
    assert (c.n <= cc.GRAPH_ROWS) == (name == "cube128")
    assert d["format"] == 3 and d["symmetric"] and d["slots"] > 0 and d["left_out"] == 0, d
    b, x0 = cc.rhs(c.n, 1)
    if name == "cube128":
        c.check_fixed(b, x0, RING_COUNTS, flavour=18)
    else:
        c.check_fixed(b, x0, RING_COUNTS, flavour=lambda k: 62 if k == 1 else 254)


@pytest.mark.parametrize("target", [16, 17])
@pytest.mark.parametrize("name", ["cube128", "past128"])
def test_cg_stops_on_a_tolerance_inside_and_at_the_end_of_a_ring_or_graph(schwz, oracle, torch_cuda, name, target):
    hp.require_extended_precision()
    c = grid_case(schwz, oracle, torch_cuda, name)
    b, x0 = cc.rhs(c.n, 1)
    c.check_stop(b, x0, target, RING_COUNTS, flavour=18 if name == "cube128" else 126)


# ---- above the threshold without a walk --------------------------------------------------------------------------------

LINES_COUNTS = (6, 17)


@pytest.mark.parametrize("name,fmt,sym,flavour", [("lines3", 3, True, 5), ("lines3_full", 3, False, 5),
                                                   ("lines3_csr", 0, False, 4), ("lines3_dict", 1, False, 4)])
def test_cg_above_the_threshold_without_a_walk(schwz, oracle, torch_cuda, name, fmt, sym, flavour):
    """1024 x 3 x 700 = 2 150 400 rows, three x lines per plane: row pairs but no canonical layout, so no walk
    and -- past 2^21 rows -- no fused direction launch: the three-launch q-free iteration with deferred x (5),
    with p.(A p) from the upper triangle or (SCHWZ_SPMV_SYM=0 at upload) from full rows; forced to plain CSR and to
    per-entry dictionaries: stored q with deferred x (4).  One reference serves the four."""
    hp.require_extended_precision()
    c = grid_case(schwz, oracle, torch_cuda, name)
    d = c.info
    assert d["format"] == fmt and d["symmetric"] == sym and d["slots"] == 0, d
    base = grid_case(schwz, oracle, torch_cuda, "lines3")
    b, x0 = cc.rhs(c.n, 1)
    c.refs = base.refs
    c.check_fixed(b, x0, LINES_COUNTS, flavour=flavour)
    if name != "lines3":
        _CASES.pop(name)   # only lines3 is used again


@pytest.mark.parametrize("levels", [0, 2])
def test_cg_on_a_variable_coefficient_matrix_past_the_threshold(schwz, oracle, torch_cuda, levels):
    """Symmetric 7-point matrix with one coefficient per edge on 130 x 130 x 125 = 2 112 500 rows: the Jacobi
    diagonal is a vector (levels = 0) or one-byte codes into a dictionary of 7 values (levels = 2, not pair coded:
    the plan keeps stored q for diag.mode == 2).  Stored q, deferred x: 4."""
    hp.require_extended_precision()
    rp, col, val = cc.variable_coefficients((130, 130, 125), levels, 7)
    n = len(rp) - 1
    assert n > cc.GRAPH_ROWS
    dg = hp.precond_jacobi(rp, col, val, np.float64)(np.ones(n))
    assert len(np.unique(dg)) == (7 if levels else n)
    c = Case(schwz, torch_cuda, "varcoef%d" % levels, rp, col, val, lambda dt: (lambda v: hp.spmv(rp, col, val, v, dt)),
             lambda dt: hp.precond_jacobi(rp, col, val, dt), diag="dict" if levels else "vector")
    d = c.info
    assert d["format"] != 3 and d["slots"] == 0, d
    b, x0 = cc.rhs(n, 8)
    c.check_fixed(b, x0, (3, 17), flavour=4)


# ---- general preconditioners -------------------------------------------------------------------------------------------

GENERAL = {"bj7": (2, 7), "bj32": (2, 32), "ilu": (3, 1), "isai": (4, 1)}


@pytest.mark.parametrize("pc", list(GENERAL))
@pytest.mark.parametrize("size", ["few_thousand", "past_the_launch_cap"])
def test_cg_with_general_preconditioners(schwz, oracle, torch_cuda, size, pc):
    """Block-Jacobi 7 and 32, ILU(0) and ISAI: 600 625 rows of the 5-point stencil (> 2048 * 256: the
    preconditioner kernels stride) and 3 500 rows of a variable-coefficient matrix (one plane of 70 x 50: after 25
    updates the residual is still far above rounding); 1, 6 and 25 updates.
    Three launches per iteration plus the application, x in the loop: flavour 0."""
    hp.require_extended_precision()
    precond, bs = GENERAL[pc]
    if size == "few_thousand":
        rp, col, val = cc.variable_coefficients((70, 50, 1), 0, 3)
    else:
        rp, col, val = cc.laplacian(oracle, (775, 775))
        assert len(rp) - 1 == 600625
    n = len(rp) - 1
    M = {dt: hp.make_precond(schwz, oracle, rp, col, val, precond, bs, dt) for dt in (LD, np.float64)}
    c = Case(schwz, torch_cuda, "%s/%s" % (size, pc), rp, col, val, lambda dt: (lambda v: hp.spmv(rp, col, val, v, dt)),
             lambda dt: M[dt], precond, bs)
    b, x0 = cc.rhs(n, 19)
    c.check_fixed(b, x0, (1, 6, 25), flavour=0)


# ---- edges of the vector kernels -----------------------------------------------------------------------------------------

def _chain(n, kind, rng):
    """Tridiagonal SPD matrix: "uniform" -- the 1-D Laplacian (row pairs, q-free, a uniform diagonal); "random" --
    random couplings in (-1, 0), diagonal in (3, 4) (plain coding, stored q, a vector diagonal)."""
    import scipy.sparse as sp
    if kind == "uniform":
        off, dg = -np.ones(max(n - 1, 0)), 2.0 * np.ones(n)
    else:
        off, dg = rng.uniform(-1, 0, max(n - 1, 0)), rng.uniform(3, 4, n)
    a = sp.diags([off, dg, off], [-1, 0, 1], shape=(n, n), format="csr")
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


@pytest.mark.parametrize("kind", ["uniform", "random"])
@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 1023, 1025, 524287, 524289])
def test_cg_sizes_at_the_edges_of_the_vector_kernels(schwz, oracle, torch_cuda, n, kind):
    """The vector kernels work on pairs of doubles (gv = grid_for((n + 1) / 2)): odd and even n around one and two
    workgroups of pairs, and either side of kMaxGrid * 256 = 524 288.  1, 2 and 9 updates (at most n); with and
    without Jacobi.  Once the Krylov space is exhausted (updates == n) the residual is rounding noise in any
    arithmetic: the iterate is compared, the residual norm is not."""
    hp.require_extended_precision()
    rng = np.random.default_rng(n)
    rp, col, val = _chain(n, kind, rng)
    b, x0 = cc.rhs(n, n + 1)
    for precond in (1, 0):
        c = Case(schwz, torch_cuda, "chain%d/%s/%s" % (n, kind, "jacobi" if precond else "none"), rp, col, val,
                 lambda dt: (lambda v: hp.spmv(rp, col, val, v, dt)),
                 lambda dt: hp.precond_jacobi(rp, col, val, dt) if precond else hp.precond_none(dt), precond,
                 diag="uniform" if kind == "uniform" else "vector")
        counts = tuple(sorted({k for k in (1, 2, 9) if k < n}))
        if counts:
            c.check_fixed(b, x0, counts, key="open")
        if n <= 3:
            c.check_fixed(b, x0, (n,), key="full", check_resn=False)


@pytest.mark.parametrize("name", ["pair_small", "csr_small", "past128"])
def test_cg_max_iters_zero_leaves_x_alone(schwz, oracle, torch_cuda, name):
    hp.require_extended_precision()
    c = grid_case(schwz, oracle, torch_cuda, name)
    b, x0 = cc.rhs(c.n, 1)
    for rtol in (0.0, 1e-8):
        got, it, rn, fl = c.device(b, x0, rtol, 0)
        assert it == 0 and np.array_equal(got, x0)
        assert fl == c.expect(rtol, 0)
        r = b.astype(LD) - c.op(LD)(x0.astype(LD))
        r_ld = float(np.sqrt(hp.dot(r, r)))
        r64 = b - c.op(np.float64)(x0)
        dev = max(abs(float(np.sqrt(hp.dot(r64, r64))) - r_ld) / r_ld, 2.0 ** -52)
        assert abs(rn - r_ld) <= MARGIN * dev * r_ld, (name, rn, r_ld)


@pytest.mark.parametrize("n", [1000, 2200001])
def test_cg_start_vector_is_the_solution_of_a_diagonal_system(schwz, torch_cuda, n):
    """Powers of two on the diagonal, integers in x0: b = D x0 holds exactly, the start residual is exactly zero and
    nothing runs, with and without a tolerance, below and past the graph threshold."""
    rng = np.random.default_rng(10)
    d = np.ldexp(1.0, rng.integers(-3, 4, n))
    x0 = rng.integers(-8, 9, n).astype(np.float64)
    b = d * x0
    A = schwz.Csr(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d)
    for precond in (0, 1):
        cg = schwz.Pcg(A, precond)
        for rtol in (0.0, 1e-6):
            d_b, d_x = _dev(torch_cuda, b), _dev(torch_cuda, x0)
            it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, 20)
            assert it == 0 and rn == 0.0
            assert np.array_equal(d_x.cpu().numpy(), x0)


# ---- stops on a tolerance, small matrices --------------------------------------------------------------------------------

@pytest.mark.parametrize("target", [5, 16, 17, 31])
@pytest.mark.parametrize("name,env", [("pair_small", {}), ("csr_small", {}), ("csr_small", {"SCHWZ_CG_DEFERX": "2"}),
                                      ("walk_small", {"SCHWZ_CG_DEFERX": "2"})])
def test_cg_stops_at_the_iteration_the_reference_stops_at(schwz, oracle, torch_cuda, name, env, target):
    """Graph replays of 16 (pair_small, csr_small), the ring of 16 forced on small matrices (stored q, and the
    walk): stops inside a ring / graph, on its last update and on the first of the next."""
    hp.require_extended_precision()
    c = grid_case(schwz, oracle, torch_cuda, name)
    b, x0 = cc.rhs(c.n, 1)
    c.check_stop(b, x0, target, SMALL_COUNTS, env=env)


@pytest.mark.parametrize("name", ["walk_small", "walk_small8", "gen520"])
def test_cg_in_the_walk_forced_on_small_grids(schwz, oracle, torch_cuda, name):
    """The matrices the child processes use for the walk's switches, under the default switches: 256 x 4 x 12 and
    256 x 8 x 12 (planes of two and four chunks), 520 x 520 (gen mode), deferred x forced: 254."""
    hp.require_extended_precision()
    c = grid_case(schwz, oracle, torch_cuda, name)
    d = c.info
    assert d["format"] == 3 and d["symmetric"] and d["slots"] > 0 and d["left_out"] == 0, d
    b, x0 = cc.rhs(c.n, 1)
    c.check_fixed(b, x0, SMALL_COUNTS, env=D2, flavour=254)


# ---- the postponed tail of a fixed-work solve ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["past128", "lines3", "walk_small", "csr_small"])
def test_cg_lazy_tail(schwz, oracle, torch_cuda, name):
    """rtol = 0 with deferred x: the last residual update and state advance are postponed until somebody asks.
    (a) Nobody asks (want_stats=False), and a second solve from another start vector follows on the same object:
    both iterates are the reference's.  (b) The statistics are asked for: the postponed launches run (with the
    last direction rebuilt first where it was never stored, cg_rebuild_direction_kernel), and the residual norm
    is the reference's -- every check_fixed of this module goes that way; here once more after (a) on the same
    object.  Walk (past128, walk_small: bit 128) and no walk (lines3: q-free, csr_small: stored q)."""
    hp.require_extended_precision()
    c = grid_case(schwz, oracle, torch_cuda, name)
    env = {} if c.n > cc.GRAPH_ROWS else {"SCHWZ_CG_DEFERX": "2"}
    counts = {"past128": RING_COUNTS, "lines3": LINES_COUNTS}.get(name, SMALL_COUNTS)
    b, x0 = cc.rhs(c.n, 1)
    ref = c.reference(b, x0, counts)
    k = 17
    got, _, _, fl = c.device(b, x0, 0.0, k, env, want_stats=False)
    assert fl == c.expect(0.0, k, env) and fl & 4 and (fl & 128 == 128) == (name in ("past128", "walk_small")), fl
    b2, x2 = cc.rhs(c.n, 77)
    ref2 = c.reference(b2, x2, (6,), key="second")
    got2, _, _, fl2 = c.device(b2, x2, 0.0, 6, env, want_stats=False)
    assert fl2 == fl
    for tag, g, r, kk in (("first", got, ref, k), ("second", got2, ref2, 6)):
        x_ld, x_64 = r[LD][0][kk], r[np.float64][0][kk]
        raw = _inf(x_64 - x_ld) / _inf(x_ld)
        dev = max(raw, kk * 2.0 ** -52)
        err = _inf(g - x_ld) / _inf(x_ld)
        RATIOS.append(("%s/lazy-%s" % (name, tag), c.n, kk, fl, dev, kk * 2.0 ** -52, err / dev, 0.0, -1.0, raw))
        assert err <= MARGIN * dev, (name, tag, err, dev)
    c.tag = name + "/lazy-stats"
    c.check_fixed(b, x0, (k,), env=env, ref_counts=counts)
    c.tag = name


def test_cg_statistics_asked_for_after_the_solve(schwz, oracle, torch_cuda):
    """The other way to the postponed launches: a subdomain's local solve whose statistics are never requested,
    then schwz_ras_last_inner_stats (pcg_last_stats).  One subdomain, 128 x 128 x 129: the local solve is CG on
    the whole matrix from y = 0 (flavour 254); iterate, iteration count and residual norm against the reference."""
    hp.require_extended_precision()
    torch = torch_cuda
    shape = cc.GRIDS["past128"][0]
    prob = schwz.Problem.laplacian(3, *shape)
    sd = schwz.Subdomain(prob, 1, 0, 2, schwz.partition_regular(prob.N, 1))
    n = sd.local_size_x
    assert n == prob.N and sd.halo_size == 0
    b, _ = cc.rhs(n, 1)
    k = 10
    sd.to_device(b, precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=k)
    idx = torch.arange(n, dtype=torch.int32, device="cuda")

    def put(which, a):
        p, cnt = sd.vector(which)
        assert cnt >= n
        t = _dev(torch, a)
        schwz.gather(n, idx.data_ptr(), t.data_ptr(), p)
        torch.cuda.synchronize()

    def get(which):
        p, cnt = sd.vector(which)
        t = torch.empty(n, dtype=torch.float64, device="cuda")
        schwz.gather(n, idx.data_ptr(), p, t.data_ptr())
        torch.cuda.synchronize()
        return t.cpu().numpy()
    put(1, b)
    put(2, np.zeros(n))
    sd.local_solve(want_iters=False)
    torch.cuda.synchronize()
    got = get(2)
    fl = sd.cg_flavour()
    assert fl == 254, fl
    it, rn = sd.last_inner_stats()
    assert it == k
    c = grid_case(schwz, oracle, torch, "past128")
    ref = c.reference(b, None, (k,), key="zero start")
    compare("past128/stats-later", n, fl, k, got, rn, ref[LD][0][k], ref[LD][1][k], ref[np.float64][0][k],
            ref[np.float64][1][k])


# ---- the switches read once per process: child processes -----------------------------------------------------------------

_CARD_LOST = []   # set by the first child that ends on a signal or a timeout: nothing more is started on the card


def _job(case, iters, rtol=0.0, env=None):
    return dict(case=case, iters=iters, rtol=rtol, env=env or {})


# id -> (environment of the child, jobs, seconds allowed, what the setting must produce: per job the flavour, or None
# for "what the plan gives", and a dict of upload properties).
SETTINGS = {
    # stored q for row pairs too: bits 0-1 clear
    "qfree0": ({"SCHWZ_CG_QFREE": "0"}, [_job("pair_small", 17), _job("walk_small", 17, env=D2), _job("lines3", 6)],
               [0, 12, 4], {}),
    # p.(A p) from full rows, hence no fused direction launch: three launches (5 with the walk's update launch: 13)
    "sym0": ({"SCHWZ_CG_SYM": "0"}, [_job("pair_small", 17), _job("past128", 17)], [1, 13], {}),
    "fusedir0": ({"SCHWZ_CG_FUSEDIR": "0"}, [_job("pair_small", 17), _job("walk_small", 17, env=D2)], [1, 13], {}),
    # the fused launch without a walk past 2^21 rows, with the ring (6) and with x in the loop (2)
    "fusedir2": ({"SCHWZ_CG_FUSEDIR": "2"}, [_job("lines3", 6), _job("lines3", 17, env=D0), _job("csr_small", 17)],
                 [6, 2, 0], {}),
    # no graph replays where they are the default: the same flavours, launched one by one
    "graph0": ({"SCHWZ_CG_GRAPH": "0"}, [_job("pair_small", 33), _job("csr_small", 33)], [2, 0], {}),
    # graphs past 2^21 rows (x in the loop): the q-free three-launch iteration and the fused walk, replayed
    "graph2": ({"SCHWZ_CG_GRAPH": "2"}, [_job("lines3", 17, env=D0), _job("past128", 33, env=D0)], [1, 18], {}),
    # byte ids only: no run-length records, hence no walk
    "rle0": ({"SCHWZ_SPMV_RLE": "0"}, [_job("past128", 17), _job("pair_small", 17)], [5, 2],
             {"past128": dict(format=3, slots=0)}),
    # records of 8 runs only: enough for the 256-row x lines of walk_small, not for the 128-row lines of past128
    # (a chunk of four lines has twelve runs), which loses its walk
    "rle8": ({"SCHWZ_SPMV_RLE": "8"}, [_job("past128", 17), _job("walk_small", 17, env=D2)], [5, 254],
             {"past128": dict(format=3, slots=0), "walk_small": dict(walk=True)}),
    # bands of the fused direction launch: planes of 2048 rows take all three heights (the default there is 1024)
    "tdir512": ({"SCHWZ_SWEEP_TDIR": "512", "SCHWZ_SWEEP_LDIR": "8"}, [_job("walk_small8", 17, env=D2)], [254],
                {"walk_small8": dict(walk=True)}),
    "tdir1024": ({"SCHWZ_SWEEP_TDIR": "1024", "SCHWZ_SWEEP_LDIR": "5"}, [_job("walk_small8", 17, env=D2)], [254],
                 {"walk_small8": dict(walk=True)}),
    "tdir2048": ({"SCHWZ_SWEEP_TDIR": "2048", "SCHWZ_SWEEP_LDIR": "3"}, [_job("walk_small8", 17, env=D2)], [254],
                 {"walk_small8": dict(walk=True)}),
    "firstpercu0": ({"SCHWZ_SWEEP_FIRSTPERCU": "0"}, [_job("walk_small", 17, env=D2), _job("walk_small8", 17, env=D2)],
                    [254, 254], {"walk_small": dict(walk=True)}),
    # whole-chunk planes only: the 520-row lines get no walk (with the default they do: test_cg_in_the_walk_...)
    "gen0": ({"SCHWZ_SWEEP_GEN": "0"}, [_job("gen520", 17, env=D2)], [6], {"gen520": dict(format=3, slots=0)}),
    # plain CSR past 2 M rows: the stream kernel with short-lived workgroups is the default; without it, with the
    # persistent form, with and without non-temporal stores of y
    "stream0": ({"SCHWZ_SPMV_STREAM": "0"}, [_job("lines3_csr", 17), _job("csr_small", 17)], [4, 0],
                {"lines3_csr": dict(format=0)}),
    "seq0": ({"SCHWZ_STREAM_SEQ": "0"}, [_job("lines3_csr", 17), _job("csr_small", 17)], [4, 0],
             {"lines3_csr": dict(format=0)}),
    "nty0": ({"SCHWZ_STREAM_NTY": "0"}, [_job("lines3_csr", 17), _job("csr_small", 17)], [4, 0],
             {"lines3_csr": dict(format=0)}),
    "nty1": ({"SCHWZ_STREAM_NTY": "1"}, [_job("lines3_csr", 17), _job("csr_small", 17)], [4, 0],
             {"lines3_csr": dict(format=0)}),
}
CHILD_COUNTS = {"past128": RING_COUNTS, "cube128": RING_COUNTS, "lines3": LINES_COUNTS}


def _reference_of_job(schwz, oracle, torch, job):
    name = job["case"]
    base = "lines3" if name.startswith("lines3") else name
    c = grid_case(schwz, oracle, torch, base)
    b, x0 = cc.rhs(c.n, 1)
    return c, c.reference(b, x0, CHILD_COUNTS.get(base, SMALL_COUNTS))


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_cg_under_a_switch_read_once_per_process(schwz, oracle, torch_cuda, tmp_path, setting):
    """One child process per setting (cg_child.py), one at a time, each with its own time limit; the parent holds
    the references and compares as everywhere in this module, and asserts the flavour and the coding the setting
    must produce."""
    hp.require_extended_precision()
    if _CARD_LOST:
        pytest.skip("an earlier child process ended on a signal or a timeout (%s)" % _CARD_LOST[0])
    env_set, jobs, flavours, props = SETTINGS[setting]
    refs = [_reference_of_job(schwz, oracle, torch_cuda, j) for j in jobs]   # before the child: it needs the card
    with open(tmp_path / "jobs.json", "w") as f:
        json.dump(jobs, f)
    env = dict(os.environ)
    env.update(env_set)
    big = len({j["case"] for j in jobs if np.prod(cc.GRIDS[j["case"]][0]) > 1000000})
    limit = 60 + 45 * big   # start-up and small solves; upload and solves of a matrix of 2 M rows
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "cg_child.py"),
                            str(tmp_path / "jobs.json"), str(tmp_path)], env=env, capture_output=True, text=True,
                           timeout=limit)
    except subprocess.TimeoutExpired:
        _CARD_LOST.append("%s: no result after %d s" % (setting, limit))
        pytest.fail(_CARD_LOST[0])
    if p.returncode < 0 or p.returncode in (134, 139, 124, 137):
        _CARD_LOST.append("%s: exit status %d" % (setting, p.returncode))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    NOTES.append("child %s: %.1f s" % (setting, time.time() - t0))
    results = json.load(open(tmp_path / "result.json"))
    assert len(results) == len(jobs)
    for j, (job, res, want, (c, ref)) in enumerate(zip(jobs, results, flavours, refs)):
        name, k = job["case"], job["iters"]
        full = dict(env_set)
        full.update(job["env"])
        planned = plan_flavour(res["n"], res["format"], res["symmetric"], res["slots"] > 0, res["left_out"] == 0,
                               job["rtol"], k, full)
        assert res["flavour"] == planned == want, (setting, name, res["flavour"], planned, want)
        for key, v in props.get(name, {}).items():
            assert (res["slots"] > 0) == v if key == "walk" else res[key] == v, (setting, name, key, res)
        assert res["iters"] == k
        got = np.load(tmp_path / ("x_%d.npy" % j))
        compare("%s/%s" % (setting, name), res["n"], res["flavour"], k, got, res["resnorm"], ref[LD][0][k], ref[LD][1][k],
                ref[np.float64][0][k], ref[np.float64][1][k])
