"""The device-resident Chebyshev iteration (csrc/chebyshev.hip) against the extended-precision restatement of
tests/hp_chebyshev.py.

The tolerance is the rule of tests/test_gpu_gmres.py and tests/test_gpu_bicgstab.py, unchanged: every case computes
the reference twice, in longdouble and (the same text) in float64, and takes dev = |x_f64 - x_ld|_inf / |x_ld|_inf as
the size of legitimate float64 rounding.  The kernel must stay within 32 * max(dev, iters * 2^-52) of the longdouble
iterate, and likewise for the residual norm.  The reference decides the tolerance; the kernel's output never does.
Every case runs without a preconditioner and with Jacobi, from a warm start x_0 != 0, with a random right-hand side,
on the solver's own default bounds (Gershgorin bound / 30, Gershgorin bound) unless it says otherwise."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hp_chebyshev
import hp_reference as hp

pytestmark = pytest.mark.gpu

LD = np.longdouble
MARGIN = 32.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
MPIEXEC = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
DRIVER = os.path.join(ROOT, "schwarz-lib_amd", "build", "cheb_driver")
PC = {"none": 0, "jacobi": 1}
BOTH = pytest.mark.parametrize("pc", ["none", "jacobi"])


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _inf(a):
    return float(np.abs(a).max()) if len(a) else 0.0


def _rhs(n, seed=29):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(n) * 0.1


def _scipy_csr(a):
    a = a.tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def lap1d_shifted(n):
    """tridiag(-1, 2, -1) + 0.1 I"""
    import scipy.sparse as sp
    return _scipy_csr(sp.diags([-np.ones(n - 1), np.full(n, 2.1), -np.ones(n - 1)], [-1, 0, 1], shape=(n, n)))


def spd_band(n, half, seed, wrap=False):
    """Symmetric band of 2 * half + 1 entries per row (fewer at the ends; wrap: the band wraps around, every row is
    full), off-diagonal values in (-1, 1), diagonal 1 + sum |off-diagonal|: strictly dominant and positive, hence
    SPD."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    a = sp.diags([rng.uniform(-1.0, 1.0, n - k) for k in range(1, half + 1)], list(range(1, half + 1)), shape=(n, n))
    if wrap:
        a = a + sp.diags([rng.uniform(-1.0, 1.0, k) for k in range(1, half + 1)],
                         [-(n - k) for k in range(1, half + 1)], shape=(n, n))
    a = (a + a.T).tocsr()
    a = a + sp.diags(1.0 + np.asarray(abs(a).sum(axis=1)).ravel())
    return _scipy_csr(a)


class Case:
    """One matrix + preconditioner on the device, and both references on the host."""

    def __init__(self, schwz, torch, rp, col, val, pc, tag, want_format=None, fallback=None):
        self.torch, self.rp, self.col, self.val = torch, rp, col, val
        self.n = len(rp) - 1
        self.tag = "%s/%s" % (tag, pc)
        self.A = schwz.Csr(rp, col, val)
        if want_format is not None:
            assert self.A.format() == want_format, (tag, self.A.format())
        if fallback is not None:     # does the tile pipeline take the matrix?
            assert (hp.stream_cap(rp) == 0) == fallback, (tag, hp.stream_cap(rp))
        self.ch = schwz.Chebyshev(self.A, PC[pc])
        self.diag = hp_chebyshev.diagonal(rp, col, val) if pc == "jacobi" else None
        self.bounds = self.ch.bounds()

    def device(self, b, x0, rtol, max_iters, want_stats=True):
        d_b, d_x = _dev(self.torch, b), _dev(self.torch, x0 if x0 is not None else np.zeros(self.n))
        it, rn = self.ch.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, max_iters, want_stats=want_stats)
        self.torch.cuda.synchronize()
        return d_x.cpu().numpy(), it, rn

    def reference(self, b, x0, iters, rtol=0.0, dtype=LD, bounds=None):
        lo, hi = bounds or self.bounds
        return hp_chebyshev.chebyshev(self.rp, self.col, self.val, b, x0, self.diag, lo, hi, iters, rtol, dtype)

    def check_fixed(self, b, x0, iters, bounds=None):
        x_ld, h_ld = self.reference(b, x0, iters, bounds=bounds)
        x_64, h_64 = self.reference(b, x0, iters, dtype=np.float64, bounds=bounds)
        assert len(h_ld) - 1 == len(h_64) - 1 == iters, self.tag
        got, it, rn = self.device(b, x0, 0.0, iters)
        assert it == iters, (self.tag, it)
        assert self.ch.last_stats() == (it, rn)
        self.compare(got, rn, x_ld, h_ld, x_64, h_64, iters)
        return got

    def compare(self, got, rn, x_ld, h_ld, x_64, h_64, iters):
        floor = max(iters, 1) * 2.0 ** -52
        scale = _inf(x_ld)
        dev_x = max(_inf(x_64.astype(LD) - x_ld) / scale, floor)
        err_x = _inf(got.astype(LD) - x_ld) / scale
        r_ld = float(h_ld[-1])
        dev_r = max(abs(float(h_64[-1]) - r_ld) / r_ld, floor)
        err_r = abs(rn - r_ld) / r_ld
        print("%s iters %d: x err %.2e = %.2f dev (dev %.2e), resn err %.2e = %.2f dev" %
              (self.tag, iters, err_x, err_x / dev_x, dev_x, err_r, err_r / dev_r))
        assert np.isfinite(got).all() and np.isfinite(rn)
        assert err_x <= MARGIN * dev_x, (self.tag, iters, err_x, dev_x)
        assert err_r <= MARGIN * dev_r, (self.tag, iters, err_r, dev_r)


# ---- 1. the smallest shapes ------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 256, 257, 513])
def test_smallest_shapes(schwz, torch_cuda, n, pc):
    """The tails and both sides of the 256-row tile.  m = 0 leaves x bit-identical; m = 1 is the start launch and the
    vector launch alone; m = 2 adds one iteration launch; m = 9 swaps the d buffers eight times."""
    b, x0 = _rhs(n)
    c = Case(schwz, torch_cuda, *lap1d_shifted(n), pc, "lap1d_%d" % n, fallback=False)
    got, it, rn = c.device(b, x0, 0.0, 0)
    assert it == 0 and np.array_equal(got, x0)
    r0 = b.astype(LD) - hp.spmv(c.rp, c.col, c.val, x0)
    assert abs(rn - float(np.sqrt(np.dot(r0, r0)))) <= 64 * 2.0 ** -52 * rn
    got, it, rn = c.device(b, x0, 0.0, 0, want_stats=False)     # nothing at all is launched
    assert np.array_equal(got, x0)
    for m in (1, 2, 9):
        c.check_fixed(b, x0, m)


# ---- 2. / 3. nonzero-limited tiles, the fallback kernel --------------------------------------------------------------

@BOTH
def test_nonzero_limited_tiles(schwz, torch_cuda, pc):
    """31 entries in every row (the band wraps around): 66 rows fill a 2048-product tile, the other 190 lanes of the
    workgroup own no row and must store nothing; the tiles start at multiples of 2046 entries, so every second one
    is two entries into its 16-byte aligned window."""
    rp, col, val = spd_band(700, 15, 31, wrap=True)
    assert np.diff(rp).min() == np.diff(rp).max() == 31 and np.diff(hp.tiles_of(rp)).max() == 66
    b, x0 = _rhs(700)
    Case(schwz, torch_cuda, rp, col, val, pc, "band31", fallback=False).check_fixed(b, x0, 12)


@BOTH
@pytest.mark.parametrize("name", ["band41", "arrow200"])
def test_fallback_kernel(schwz, torch_cuda, name, pc):
    """A row longer than the largest masked-add count (32) sends the matrix to the row-per-lane kernels."""
    if name == "band41":
        rp, col, val = spd_band(300, 20, 41)
        assert np.diff(rp).max() == 41
    else:
        rp, col, val = hp.arrow_matrix(200, np.random.default_rng(200))
        assert np.diff(rp).max() == 200
    n = len(rp) - 1
    b, x0 = _rhs(n)
    Case(schwz, torch_cuda, rp, col, val, pc, name, fallback=True).check_fixed(b, x0, 12)


# ---- 4. / 5. coded matrices, a general matrix ------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("shape", [(16, 10, 7), (12, 12, 12)])
def test_coded_matrices(schwz, oracle, torch_cuda, monkeypatch, shape, pc):
    """The SpMV of these matrices is row-pair coded (format 3; at these sizes the upload would choose the per-entry
    dictionary, format 1, so the pair coding is switched on the way tests/test_gpu_bicgstab.py does); the solver reads
    their plain CSR.  40 corrections: several workgroups and 39 swaps of the d buffers -- a solver that updated d in
    place fails here."""
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
    rp, col, val = oracle.laplacian3d(*shape)
    n = len(rp) - 1
    assert os.path.exists(os.path.join(G, "lap3d_%dx%dx%d.npz" % shape))
    b, x0 = _rhs(n)
    Case(schwz, torch_cuda, rp, col, val, pc, "lap3d_%dx%dx%d" % shape, want_format=3).check_fixed(b, x0, 40)


@BOTH
def test_general_matrix(schwz, torch_cuda, pc):
    g = np.load(os.path.join(G, "ani4_crop.npz"))
    rp, col, val = g["rp"].astype(np.int32), g["col"].astype(np.int32), g["val"].astype(np.float64)
    b, x0 = _rhs(len(rp) - 1)
    Case(schwz, torch_cuda, rp, col, val, pc, "ani4_crop").check_fixed(b, x0, 25)


# ---- 6. striding -----------------------------------------------------------------------------------------------------

_lap81 = {}


@BOTH
def test_past_the_grid_cap(schwz, oracle, torch_cuda, pc):
    """81^3 = 531 441 rows > kMaxGrid * kBlock = 2048 * 256 = 524 288: the grids of the row-per-lane kernels (the
    vector launch x += d of every fixed-work solve, the bound kernel at creation, the fallback kernels) are capped
    there and their first 7153 lanes make a second trip.  The tile pipeline runs 2076 tiles in 696 workgroups of 3
    (its grid is capped only beyond 6144 tiles, where workgroups take longer runs of tiles of the same loop).  The
    bound kernel's result is pinned below."""
    if not _lap81:
        _lap81["m"] = oracle.laplacian3d(81, 81, 81)
        _lap81["b"] = _rhs(531441)
    rp, col, val = _lap81["m"]
    n = len(rp) - 1
    assert n == 531441 > 2048 * 256
    b, x0 = _lap81["b"]
    c = Case(schwz, torch_cuda, rp, col, val, pc, "lap3d_81")
    assert c.bounds[1] == (2.0 if pc == "jacobi" else 12.0)
    c.check_fixed(b, x0, 4)


# ---- 7. bounds -------------------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("name", ["band31", "arrow200", "ani4_crop"])
def test_default_bounds_are_gershgorin(schwz, torch_cuda, name, pc):
    if name == "band31":
        rp, col, val = spd_band(700, 15, 31, wrap=True)
    elif name == "arrow200":
        rp, col, val = hp.arrow_matrix(200, np.random.default_rng(200))
    else:
        g = np.load(os.path.join(G, "ani4_crop.npz"))
        rp, col, val = g["rp"].astype(np.int32), g["col"].astype(np.int32), g["val"].astype(np.float64)
    ch = schwz.Chebyshev(schwz.Csr(rp, col, val), PC[pc])
    want = hp_chebyshev.gershgorin(rp, col, val, hp_chebyshev.diagonal(rp, col, val) if pc == "jacobi" else None)
    lo, hi = ch.bounds()
    assert abs(hi - want) <= 4 * np.spacing(want), (hi, want)
    assert lo == hi / 30.0


@BOTH
def test_set_bounds_takes_effect_and_the_object_is_reused(schwz, torch_cuda, pc):
    rp, col, val = spd_band(700, 15, 31, wrap=True)
    b, x0 = _rhs(700)
    c = Case(schwz, torch_cuda, rp, col, val, pc, "band31/bounds")
    lo, hi = c.bounds
    first = c.check_fixed(b, x0, 7)
    other = (hi / 8.0, hi * 1.25)
    c.ch.set_bounds(*other)
    assert c.ch.bounds() == other
    second = c.check_fixed(b, x0, 7, bounds=other)
    assert not np.array_equal(first, second)
    c.check_fixed(b, x0, 3, bounds=other)
    for bad in ((0.0, 1.0), (-1.0, 1.0), (1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.5, float("inf"))):
        with pytest.raises(schwz.SchwzError) as e:
            c.ch.set_bounds(*bad)
        assert e.value.code == schwz.capi.ERR_INVALID
    assert c.ch.bounds() == other
    c.ch.set_bounds(lo, hi)
    assert np.array_equal(c.check_fixed(b, x0, 7), first)


@pytest.mark.parametrize("bad", [0.0, -2.0, float("inf"), None])
def test_jacobi_needs_a_positive_diagonal(schwz, torch_cuda, bad):
    import scipy.sparse as sp
    n = 300
    a = sp.diags([-np.ones(n - 1), np.full(n, 2.0), -np.ones(n - 1)], [-1, 0, 1], shape=(n, n)).tolil()
    if bad is None:
        a[257, 257] = 0.0
        a = a.tocsr()
        a.eliminate_zeros()          # the diagonal entry of row 257 is not stored
    else:
        a[257, 257] = bad
    rp, col, val = _scipy_csr(a)
    A = schwz.Csr(rp, col, val)
    with pytest.raises(schwz.SchwzError) as e:
        schwz.Chebyshev(A, schwz.capi.PRECOND_JACOBI)
    assert e.value.code == schwz.capi.ERR_NOT_SPD
    assert "row 257" in str(e.value)
    if bad is None or bad == 0.0 or bad == -2.0:
        schwz.Chebyshev(A, schwz.capi.PRECOND_NONE)     # without Jacobi the diagonal is not looked at


# ---- 8. tolerance stops ----------------------------------------------------------------------------------------------

GAP = 1.2


def _find_stop(c, b, x0, k):
    """rtol for which the solve stops at the checked iterate k: rtol * nu is the geometric mean of the norm that is to
    stop the solve and the smallest norm at any earlier checked iterate, the two at least a factor GAP apart (rounding
    moves these norms by about 1e-13 relative)."""
    every = hp_chebyshev.CHECK_EVERY
    assert k % every == 0 and k > 0
    _, h = c.reference(b, x0, k)
    h = [float(v) for v in h]
    earlier = min(h[j] for j in range(0, k, every))
    assert h[k] * GAP <= earlier, "no clear gap at iterate %d: take another right-hand side" % k
    return float(np.sqrt(h[k] * earlier) / h[0]), h


@BOTH
@pytest.mark.parametrize("k", [8, 16])
def test_tolerance_stop_at_a_checked_iterate(schwz, oracle, torch_cuda, k, pc):
    """lap2d_64: the solve returns x_k for the first checked k that passes.  A solve given a larger max_iters than
    needed (200: three polling chunks of launches that must change nothing) returns the same bits as one given exactly
    the stopping count.  At k = 8 the norm is below the threshold from k = 5 on: the solve still reports 8."""
    rp, col, val = oracle.laplacian2d(64)
    b, x0 = _rhs(len(rp) - 1)
    c = Case(schwz, torch_cuda, rp, col, val, pc, "lap2d_64/stop%d" % k)
    rtol, h = _find_stop(c, b, x0, k)
    if k == 8:
        assert h[7] <= rtol * h[0] < h[0]
    x_ld, h_ld = c.reference(b, x0, 200, rtol)
    x_64, h_64 = c.reference(b, x0, 200, rtol, dtype=np.float64)
    assert len(h_ld) - 1 == len(h_64) - 1 == k
    x_long, it_long, rn_long = c.device(b, x0, rtol, 200)
    assert c.ch.last_stats() == (it_long, rn_long)
    x_short, it_short, rn_short = c.device(b, x0, rtol, k)
    assert it_long == it_short == k
    assert np.array_equal(x_long, x_short)
    assert rn_long == rn_short
    c.compare(x_long, rn_long, x_ld, h_ld, x_64, h_64, k)


@BOTH
def test_tolerance_without_a_stop_runs_max_iters(schwz, oracle, torch_cuda, pc):
    """max_iters = 13 with the tolerance that would stop at 16: iterate 8 is checked and does not pass, iterate 13 is
    the last one whatever its norm is."""
    rp, col, val = oracle.laplacian2d(64)
    b, x0 = _rhs(len(rp) - 1)
    c = Case(schwz, torch_cuda, rp, col, val, pc, "lap2d_64/nostop")
    rtol, _ = _find_stop(c, b, x0, 16)
    x_ld, h_ld = c.reference(b, x0, 13, rtol)
    x_64, h_64 = c.reference(b, x0, 13, rtol, dtype=np.float64)
    assert len(h_ld) - 1 == len(h_64) - 1 == 13
    got, it, rn = c.device(b, x0, rtol, 13)
    assert it == 13
    c.compare(got, rn, x_ld, h_ld, x_64, h_64, 13)
    # the same corrections as the fixed-work solve, launched differently: the same bits
    fixed, it, _ = c.device(b, x0, 0.0, 13)
    assert it == 13 and np.array_equal(got, fixed)


@BOTH
def test_zero_start_residual_stops_at_zero(schwz, torch_cuda, pc):
    """Small integer data: b = A x0 holds exactly in float64 in any order, so ||r_0|| == 0.0: no correction, x
    untouched."""
    import scipy.sparse as sp
    n = 1000
    rng = np.random.default_rng(10)
    off = rng.integers(-3, 4, n - 1)
    a = sp.diags([off, rng.integers(8, 12, n), off], [-1, 0, 1], shape=(n, n), format="csr").astype(np.float64)
    x0 = rng.integers(-8, 9, n).astype(np.float64)
    b = a @ x0
    c = Case(schwz, torch_cuda, *_scipy_csr(a), pc, "int1000")
    got, it, rn = c.device(b, x0, 1e-6, 20)
    assert it == 0 and rn == 0.0
    assert np.array_equal(got, x0)
    assert c.ch.last_stats() == (0, 0.0)


# ---- 9. the lazy norm ------------------------------------------------------------------------------------------------

@BOTH
def test_lazy_norm(schwz, torch_cuda, pc):
    """A fixed-work solve that was not asked for its norm computes it when last_stats asks: once, storing nothing."""
    torch = torch_cuda
    rp, col, val = spd_band(700, 15, 31, wrap=True)
    b, x0 = _rhs(700)
    c = Case(schwz, torch, rp, col, val, pc, "band31/lazy")
    m = 9
    x_ld, h_ld = c.reference(b, x0, m)
    x_64, h_64 = c.reference(b, x0, m, dtype=np.float64)
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    assert c.ch.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, m, want_stats=False) == (0, 0.0)   # (nothing was asked)
    torch.cuda.synchronize()
    before = d_x.cpu().numpy()
    first = c.ch.last_stats()
    mid = d_x.cpu().numpy()
    second = c.ch.last_stats()
    after = d_x.cpu().numpy()
    assert first == second and first[0] == m
    assert np.array_equal(before, mid) and np.array_equal(mid, after)
    c.compare(after, first[1], x_ld, h_ld, x_64, h_64, m)
    # the same number as a solve that asks at once
    got, it, rn = c.device(b, x0, 0.0, m)
    assert (it, rn) == first and np.array_equal(got, after)


# ---- 10. inside a subdomain ------------------------------------------------------------------------------------------

def test_subdomain_step_is_the_reference(schwz, oracle, torch_cuda):
    """One local solve of a subdomain with a neighbour (overlap rows, a halo) is the Chebyshev iteration on the local
    matrix with b~ and the start vector y.  The setter round-trips, the getters answer as documented, and CG comes
    back exactly."""
    torch, c = torch_cuda, schwz.capi
    rp, col, val = oracle.laplacian3d(16, 10, 7)
    P, me, m = 2, 1, 6
    prob = schwz.Problem.from_csr(rp, col, val)
    sd = schwz.Subdomain(prob, P, me, 2, schwz.partition_regular(prob.N, P))
    nloc = sd.local_size_x
    assert sd.overlap_size > 0 and sd.halo_size > 0
    rng = np.random.default_rng(5)
    sd.to_device(rng.standard_normal(nloc), precond=c.PRECOND_JACOBI, local_tol=0.0, local_max_iters=m)
    cg_answers = (sd.early_pack_ok(), sd.cg_flavour(), sd.y_form())
    cg_bytes = sd.algorithmic_bytes(1)
    assert sd.sym_solver() == c.SYM_CG
    with pytest.raises(schwz.SchwzError) as e:
        sd.cheb_bounds()
    assert e.value.code == c.ERR_INVALID
    lrp, lcol, lval = sd.local_matrix()
    diag = hp_chebyshev.diagonal(lrp, lcol, lval)
    nx = nloc + sd.halo_size
    idx = torch.arange(nx, dtype=torch.int32, device="cuda")

    def get(which):
        p, cnt = sd.vector(which)
        t = torch.empty(cnt, dtype=torch.float64, device="cuda")
        schwz.gather(cnt, idx.data_ptr(), p, t.data_ptr())
        torch.cuda.synchronize()
        return t.cpu().numpy()

    def put(which, a):
        p, cnt = sd.vector(which)
        assert len(a) == cnt
        t = _dev(torch, a)
        schwz.gather(cnt, idx.data_ptr(), t.data_ptr(), p)
        torch.cuda.synchronize()

    def check_step(seed):
        put(0, np.random.default_rng(seed).standard_normal(nx))
        put(2, np.random.default_rng(seed + 1).standard_normal(nloc) * 0.1)
        sd.update_boundary()
        torch.cuda.synchronize()
        bt, y0 = get(1), get(2)
        lo, hi = sd.cheb_bounds()
        assert abs(hi - hp_chebyshev.gershgorin(lrp, lcol, lval, diag)) <= 4 * np.spacing(hi) and lo == hi / 30.0
        assert sd.local_solve(want_iters=True) == m
        torch.cuda.synchronize()
        y = get(2)
        x_ld, h_ld = hp_chebyshev.chebyshev(lrp, lcol, lval, bt, y0, diag, lo, hi, m)
        x_64, h_64 = hp_chebyshev.chebyshev(lrp, lcol, lval, bt, y0, diag, lo, hi, m, dtype=np.float64)
        scale = _inf(x_ld)
        dev_x = max(_inf(x_64.astype(LD) - x_ld) / scale, m * 2.0 ** -52)
        err_x = _inf(y.astype(LD) - x_ld) / scale
        it, rn = sd.last_inner_stats()
        dev_r = max(abs(float(h_64[-1]) - float(h_ld[-1])) / float(h_ld[-1]), m * 2.0 ** -52)
        err_r = abs(rn - float(h_ld[-1])) / float(h_ld[-1])
        print("subdomain step: y err %.2f dev, norm err %.2f dev" % (err_x / dev_x, err_r / dev_r))
        assert it == m and err_x <= MARGIN * dev_x and err_r <= MARGIN * dev_r
        assert np.array_equal(get(1), bt)

    def set_chebyshev():
        sd.set_sym_solver(c.SYM_CHEBYSHEV)
        assert sd.sym_solver() == c.SYM_CHEBYSHEV
        assert (sd.early_pack_ok(), sd.cg_flavour(), sd.y_form()) == (0, 0, 0)
        nnz = int(lrp[-1])
        assert sd.algorithmic_bytes(1) == 12 * nnz + 4 * (nloc + 1) + 56 * nloc

    set_chebyshev()
    sd.set_sym_solver(c.SYM_CHEBYSHEV)     # twice is once
    with pytest.raises(schwz.NotImplementedSchwz):
        sd.set_local_precision(c.PRECISION_F32)
    with pytest.raises(schwz.SchwzError) as e:
        sd.set_sym_solver(2)
    assert e.value.code == c.ERR_INVALID
    check_step(100)
    # the two-stage cap takes effect at the next solve
    sd.set_local_max_iters(3)
    m = 3
    check_step(110)
    sd.set_local_max_iters(6)
    m = 6
    # CG and back
    sd.set_sym_solver(c.SYM_CG)
    assert sd.sym_solver() == c.SYM_CG
    assert (sd.early_pack_ok(), sd.cg_flavour(), sd.y_form()) == cg_answers
    assert sd.algorithmic_bytes(1) == cg_bytes
    put(0, np.random.default_rng(7).standard_normal(nx))
    put(2, np.random.default_rng(8).standard_normal(nloc) * 0.1)
    sd.update_boundary()
    torch.cuda.synchronize()
    bt, y0 = get(1), get(2)
    assert sd.local_solve(want_iters=True) == 6
    torch.cuda.synchronize()
    y_cg = get(2)
    # (a fresh subdomain that never saw Chebyshev gives the same bits)
    sd2 = schwz.Subdomain(prob, P, me, 2, schwz.partition_regular(prob.N, P))
    sd2.to_device(np.random.default_rng(5).standard_normal(nloc), precond=c.PRECOND_JACOBI, local_tol=0.0,
                  local_max_iters=6)
    for which, a in ((0, np.random.default_rng(7).standard_normal(nx)), (2, y0)):
        p, cnt = sd2.vector(which)
        t = _dev(torch, a)
        schwz.gather(cnt, idx.data_ptr(), t.data_ptr(), p)
    torch.cuda.synchronize()
    sd2.update_boundary()
    sd2.local_solve()
    torch.cuda.synchronize()
    p, cnt = sd2.vector(2)
    t = torch.empty(cnt, dtype=torch.float64, device="cuda")
    schwz.gather(cnt, idx.data_ptr(), p, t.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), y_cg)
    set_chebyshev()
    check_step(120)
    # what the setter refuses
    for kw in (dict(precond=c.PRECOND_ILU), dict(precond=c.PRECOND_BLOCK_JACOBI, precond_block_size=4),
               dict(local_solver=c.SOLVER_DIRECT), dict(precond=c.PRECOND_JACOBI, non_symmetric=True)):
        sd3 = schwz.Subdomain(prob, P, me, 2, schwz.partition_regular(prob.N, P))
        sd3.to_device(np.ones(nloc), **kw)
        with pytest.raises(schwz.NotImplementedSchwz):
            sd3.set_sym_solver(c.SYM_CHEBYSHEV)
        assert sd3.sym_solver() == c.SYM_CG
        sd3.set_sym_solver(c.SYM_CG)
    sd4 = schwz.Subdomain(prob, P, me, 2, schwz.partition_regular(prob.N, P))
    sd4.to_device(np.ones(nloc), precond=c.PRECOND_BLOCK_JACOBI, precond_block_size=1)
    sd4.set_local_precision(c.PRECISION_F32)
    with pytest.raises(schwz.NotImplementedSchwz):
        sd4.set_sym_solver(c.SYM_CHEBYSHEV)
    sd4.set_local_precision(c.PRECISION_F64)
    sd4.set_sym_solver(c.SYM_CHEBYSHEV)       # block-jacobi with block size 1 counts as Jacobi
    assert sd4.algorithmic_bytes(1) == 12 * int(lrp[-1]) + 4 * (nloc + 1) + 56 * nloc


# ---- 11. a whole RAS run ---------------------------------------------------------------------------------------------

def _ras_replay(solver, rhs, tol, inner, max_iters):
    """RAS on the host, in float64, with hp_chebyshev on the subdomains' host matrices: per outer iteration the
    overlap and halo entries of every x~ take their owners' values, b~ = b - (interface matrix) x~ on the overlap rows,
    the convergence check sums the local residual norms ||b~ - A_loc x~|| (relative to the first sum), then every
    subdomain runs `inner` corrections from its own previous y and writes its interior rows back."""
    sds = solver.subdomains
    N = len(rhs)
    xg = np.zeros(N)
    loc = {}
    for me, sd in sds.items():
        lrp, lcol, lval = sd.local_matrix()
        loc[me] = dict(A=(lrp, lcol, lval), I=sd.interface_matrix(), l2g=np.asarray(sd.local_to_global),
                       n=sd.local_size_x, L=sd.local_size, y=np.zeros(sd.local_size_x),
                       diag=hp_chebyshev.diagonal(lrp, lcol, lval), bounds=sd.cheb_bounds())
    hist = {me: [] for me in sds}
    g0 = None
    for it in range(max_iters):
        bts = {}
        for me, d in loc.items():
            n, l2g = d["n"], d["l2g"]
            xs = np.zeros(N)
            xs[l2g] = xg[l2g]
            bt = rhs[l2g[:n]] - hp.spmv(*d["I"], xs, np.float64)
            bts[me] = bt
            r = bt - hp.spmv(*d["A"], xg[l2g[:n]], np.float64)
            hist[me].append(float(np.sqrt(np.dot(r, r))))
        g = sum(h[-1] for h in hist.values())
        g0 = g if g0 is None else g0
        if g / g0 <= tol:
            return it, hist, xg
        new = xg.copy()
        for me, d in loc.items():
            lo, hi = d["bounds"]
            y, _ = hp_chebyshev.chebyshev(*d["A"], bts[me], d["y"], d["diag"], lo, hi, inner, 0.0, np.float64)
            d["y"] = y
            new[d["l2g"][:d["L"]]] = y[:d["L"]]
        xg = new
    return max_iters, hist, xg


def test_ras_run_with_chebyshev_local_solves(schwz, oracle, torch_cuda):
    """P = 3 z-slabs of lap3d_12x12x12, overlap 2, Jacobi, 10 corrections per local solve on the default bounds,
    to 1e-8.  The expected history is the host replay's; on the CPU it converges in 28 outer iterations (the same
    replay with CG(10) as the local solver takes 23, like the oracle)."""
    shape, P = (12, 12, 12), 3
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=shape, overlap=2)
    m = schwz.Metadata(num_subdomains=P, symmetric_solver="chebyshev", local_precond="block-jacobi",
                       precond_max_block_size=1, local_solver_tolerance=0.0, local_max_iters=10, tolerance=1e-8,
                       max_iters=100)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    assert all(sd.sym_solver() == schwz.capi.SYM_CHEBYSHEV for sd in solver.subdomains.values())
    for sd in solver.subdomains.values():
        lo, hi = sd.cheb_bounds()
        assert hi == 2.0 and lo == 2.0 / 30.0
    rp, col, val = oracle.laplacian3d(*shape)
    N = len(rp) - 1
    want_iters, hist, x_replay = _ras_replay(solver, np.ones(N), 1e-8, 10, 100)
    out = solver.run()
    got = m.post_process_data["global_residual_vector_out"]
    print("RAS with Chebyshev(10): %d outer iterations, replay %d" % (out["iter_count"], want_iters))
    assert out["converged"] and out["iter_count"] == want_iters
    assert want_iters < 100
    for me in range(P):
        for k in range(6):
            assert abs(got[me][k] - hist[me][k]) <= 1e-10 * hist[me][k], (me, k, got[me][k], hist[me][k])
    import scipy.sparse as sp
    A = sp.csr_matrix((val, col, rp), shape=(N, N)).toarray()
    ev = np.linalg.eigvalsh(A)
    cond = float(ev[-1] / ev[0])
    x = np.linalg.solve(A, np.ones(N))
    err = np.abs(out["solution"] - x).max() / np.abs(x).max()
    print("cond %.3g, solution error %.2e" % (cond, err))
    assert err <= cond * 1e-8


def test_default_settings_keep_cg(schwz, torch_cuda):
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(8, 8, 8))
    m = schwz.Metadata(num_subdomains=2, local_precond="block-jacobi", precond_max_block_size=1, max_iters=5)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(2), quiet=True)
    solver.initialize()
    assert all(sd.sym_solver() == schwz.capi.SYM_CG for sd in solver.subdomains.values())


def test_explicit_bounds_reach_the_subdomains(schwz, torch_cuda):
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(8, 8, 8))
    m = schwz.Metadata(num_subdomains=2, symmetric_solver="chebyshev", chebyshev_eig_ratio=10.0,
                       chebyshev_lambda_max=2.5, local_max_iters=4, local_solver_tolerance=0.0, max_iters=5)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(2), quiet=True)
    solver.initialize()
    assert all(sd.cheb_bounds() == (0.25, 2.5) for sd in solver.subdomains.values())


# ---- 12. the C++ mirror ----------------------------------------------------------------------------------------------

def _driver(nranks, *args):
    if not os.path.exists(DRIVER):
        pytest.skip("cheb_driver not built (`make -C schwarz-lib_amd cheb_driver`, needs MPI)")
    if not os.path.exists(MPIEXEC):
        pytest.skip("no mpiexec on this machine")
    cmd = [MPIEXEC, "-n", str(nranks), DRIVER] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_mirror_runs_chebyshev_like_the_python_host(schwz, torch_cuda):
    P, n = 2, 32
    p = _driver(P, "chebyshev", n, 1e-8, 400, 10)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "(Chebyshev)" in p.stdout and "restart iter" not in p.stdout
    res = re.search(r"RESULT iters=(\d+) solnorm=([0-9.eE+-]+)", p.stdout)
    final = re.search(r"^ residual norm ([0-9.eE+-]+)$", p.stdout, re.M)
    assert res and final, p.stdout
    s = schwz.Settings(overlap=2)
    s.convergence_settings.enable_global_check = True
    m = schwz.Metadata(num_subdomains=P, oned_laplacian_size=n, symmetric_solver="chebyshev",
                       local_precond="block-jacobi", precond_max_block_size=1, local_solver_tolerance=0.0,
                       local_max_iters=10, tolerance=1e-8, max_iters=400)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    out = solver.run()
    assert out["converged"]
    assert int(res.group(1)) == out["iter_count"]
    print("mirror: %s iterations, final residual %s; python host: %d, %.17g" %
          (res.group(1), final.group(1), out["iter_count"], out["residual_norm"]))
    assert abs(float(final.group(1)) - out["residual_norm"]) <= 1e-10 * out["residual_norm"]
    norm = float(np.linalg.norm(out["solution"]))
    assert abs(float(res.group(2)) - norm) <= 1e-10 * norm


def test_mirror_refuses_an_unknown_solver_name():
    p = _driver(1, "sor", 8, 1e-8, 10, 4)
    assert p.returncode == 3, p.stdout + p.stderr
    assert "REFUSED" in p.stdout
