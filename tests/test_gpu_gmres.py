"""Device-resident GMRES (csrc/gmres.hip) against the extended-precision restatement of hp_reference.py:
fixed iteration counts from 7 workgroups to the grid-stride regime (n > 524 288: every streaming kernel loops
and all 2048 partial sums of a dot product are in use), matrices stored in coded formats, and the branches a
well-behaved solve never takes (exact and near breakdown, restart > n, max_iters = 0, a zero start residual,
a tolerance stop on the last vector of a cycle with its speculative extra cycle, a second solve on one object).

Tolerance of the iterate comparisons.  There is no useful a-priori bound for GMRES iterates, so every case
computes the reference twice, in longdouble and (the same text) in float64, and takes
dev = |x_f64 - x_ld|_inf / |x_ld|_inf as the size of legitimate float64 rounding.  The kernel must stay within
32 * max(dev, iters * 2^-52) of the longdouble iterate (and likewise for the residual norm): 32 because the
kernel folds its dot products from up to 2048 per-workgroup partial sums while numpy sums pairwise -- two
legitimate float64 orders whose errors differ by a small factor -- and the floor keeps a lucky dev from making
the test flaky.  The reference decides the tolerance; the kernel's output never does."""
import numpy as np
import pytest

import hp_reference as hp

pytestmark = pytest.mark.gpu

LD = np.longdouble
MARGIN = 32.0
RATIOS = []   # (case, iters, x err / dev, resn err / dev, dev x, dev resn, unfloored dev x): for tools/hp_reference_probe.py


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _inf(a):
    return float(np.abs(a).max()) if len(a) else 0.0


class Case:
    """One matrix + preconditioner + restart on the device, and both references on the host."""

    def __init__(self, schwz, oracle, torch, rp, col, val, precond, bs, restart, tag, want_format=None):
        self.torch, self.rp, self.col, self.val = torch, rp, col, val
        self.n = len(rp) - 1
        self.restart, self.tag = restart, tag
        self.A = schwz.Csr(rp, col, val)
        if want_format is not None:
            assert self.A.format() == want_format, (tag, self.A.format())
        self.gm = schwz.Gmres(self.A, precond, bs, restart)
        self.M = {dt: hp.make_precond(schwz, oracle, rp, col, val, precond, bs, dt) for dt in (LD, np.float64)}

    def device(self, b, x0, rtol, max_iters, gm=None):
        d_b = _dev(self.torch, b)
        d_x = _dev(self.torch, x0 if x0 is not None else np.zeros(self.n))
        it, rn = (gm or self.gm).solve(d_b.data_ptr(), d_x.data_ptr(), rtol, max_iters)
        return d_x.cpu().numpy(), it, rn

    def reference(self, b, x0, iters, rtol=0.0, dtype=LD):
        return hp.gmres(self.rp, self.col, self.val, b, x0, self.M[dtype], iters, self.restart, rtol, dtype)

    def check_fixed(self, b, x0, iters):
        x_ld, h_ld = self.reference(b, x0, iters)
        x_64, h_64 = self.reference(b, x0, iters, dtype=np.float64)
        got, it, rn = self.device(b, x0, 0.0, iters)
        assert it == iters == len(h_ld) - 1, (self.tag, it)
        self.compare(got, rn, x_ld, h_ld, x_64, h_64, iters)

    def compare(self, got, rn, x_ld, h_ld, x_64, h_64, iters):
        floor = iters * 2.0 ** -52
        scale = _inf(x_ld)
        raw_x = _inf(x_64.astype(LD) - x_ld) / scale
        dev_x = max(raw_x, floor)
        err_x = _inf(got.astype(LD) - x_ld) / scale
        r_ld = float(h_ld[-1])
        if r_ld == 0.0:   # an exact breakdown in exact data (n = 1): nothing to scale by, and nothing to round
            assert rn == 0.0 and float(h_64[-1]) == 0.0
            r_ld = 1.0
        dev_r = max(abs(float(h_64[-1]) - r_ld) / r_ld, floor)
        err_r = abs(rn - r_ld) / r_ld
        RATIOS.append((self.tag, iters, err_x / dev_x, err_r / dev_r, dev_x, dev_r, raw_x))
        print("%s iters %d: x err %.2e = %.2f dev (dev %.2e), resn err %.2e = %.2f dev" %
              (self.tag, iters, err_x, err_x / dev_x, dev_x, err_r, err_r / dev_r))
        assert np.isfinite(got).all()
        assert err_x <= MARGIN * dev_x, (self.tag, iters, err_x, dev_x)
        assert err_r <= MARGIN * dev_r, (self.tag, iters, err_r, dev_r)


def _rhs(n, seed=29):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(n) * 0.1


PC = {"none": (0, 1), "jacobi": (1, 1), "bj8": (2, 8), "ilu": (3, 1)}


# ---- fixed iteration counts ---------------------------------------------------------------------------------

@pytest.mark.parametrize("pc", ["none", "jacobi", "bj8", "ilu"])
@pytest.mark.parametrize("restart", [1, 4, 30])
def test_gmres_fixed_iterations_convdiff_40(schwz, oracle, torch_cuda, convdiff, restart, pc):
    rp, col, val = convdiff(40)
    b, x0 = _rhs(len(rp) - 1)
    c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], restart, "convdiff40/%s/r%d" % (pc, restart))
    for iters in (1, 5, 23):
        c.check_fixed(b, x0, iters)


# n = 600 625 > 524 288 = kMaxGrid * kBlock: gm_grid() is capped, the vector kernels stride, nparts == kMaxGrid.
# The 80-bit reference costs seconds per case at this size: six cases instead of the cross product.
LARGE = [("none", 30, 23), ("none", 1, 5), ("jacobi", 4, 5), ("jacobi", 30, 5), ("bj8", 4, 5), ("ilu", 4, 5)]


@pytest.mark.parametrize("pc,restart,iters", LARGE)
def test_gmres_fixed_iterations_past_the_grid_cap(schwz, oracle, torch_cuda, convdiff, pc, restart, iters):
    rp, col, val = convdiff(775)
    n = len(rp) - 1
    assert n == 600625 and n > 2048 * 256
    b, x0 = _rhs(n)
    c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], restart, "convdiff775/%s/r%d" % (pc, restart))
    c.check_fixed(b, x0, iters)


@pytest.mark.parametrize("pc", ["none", "jacobi", "bj8", "ilu"])
@pytest.mark.parametrize("coding", ["lap3d_pairs", "lap2d_dictionary"])
def test_gmres_fixed_iterations_on_coded_matrices(schwz, oracle, torch_cuda, monkeypatch, coding, pc):
    """Row-pair and dictionary coded matrices send the residual start (kSpmvResidInit) and the stop-aware
    product (kSpmvDot with stop_iter) through other kernels than plain CSR does."""
    if coding == "lap3d_pairs":
        monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
        monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
        rp, col, val = oracle.laplacian3d(24, 20, 17)
        want = 3
    else:
        monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "0")
        monkeypatch.setenv("SCHWZ_SPMV_PAIR", "0")
        monkeypatch.setenv("SCHWZ_SPMV_DICT", "2")
        rp, col, val = oracle.laplacian2d(90)
        want = 1
    rp, col, val = np.asarray(rp, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64)
    b, x0 = _rhs(len(rp) - 1, 31)
    for restart in (4, 30):
        c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], restart, "%s/%s/r%d" % (coding, pc, restart),
                 want_format=want)
        for iters in (1, 5, 23):
            c.check_fixed(b, x0, iters)


def _ragged(n, rng):
    """Random non-symmetric rows of 1 to 12 entries (every seventh row the diagonal alone), strictly
    diagonally dominant."""
    import scipy.sparse as sp
    rows, cols = [], []
    for i in range(n):
        k = 0 if i % 7 == 3 else int(rng.integers(1, 12))
        c = np.setdiff1d(rng.choice(n, size=k, replace=False), [i])
        rows += [i] * (len(c) + 1)
        cols += [i] + c.tolist()
    v = rng.standard_normal(len(rows))
    a = sp.csr_matrix((v, (rows, cols)), shape=(n, n))
    a.setdiag(0)
    a = (a + sp.diags(np.asarray(abs(a).sum(axis=1)).ravel() + rng.uniform(0.5, 1.5, n))).tocsr()
    a.sort_indices()
    assert (np.diff(a.indptr) == 1).sum() >= n // 8
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


@pytest.mark.parametrize("pc", ["none", "jacobi", "bj8", "ilu"])
def test_gmres_fixed_iterations_on_a_ragged_matrix(schwz, oracle, torch_cuda, pc):
    rp, col, val = _ragged(3001, np.random.default_rng(12))
    b, x0 = _rhs(len(rp) - 1, 13)
    for restart in (1, 4, 30):
        c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], restart, "ragged/%s/r%d" % (pc, restart))
        for iters in (1, 5, 23):
            c.check_fixed(b, x0, iters)


# ---- edges ------------------------------------------------------------------------------------------------------

def _diag_csr(d):
    n = len(d)
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(d, dtype=np.float64)


def test_gmres_exact_breakdown_at_the_first_vector(schwz, torch_cuda):
    """A = 2 I, b = +-1 on n = 4^10 rows: beta = 1024 and every intermediate is a dyadic number that float64 holds
    exactly in any summation order, so w - h v_0 is exactly zero: hn == 0, v_1 = 0, c = 1, s = 0, the rotated
    residual is 0 and the solve stops after one vector with x = b / 2 exactly."""
    torch = torch_cuda
    n = 4 ** 10
    b = np.random.default_rng(1).choice([-1.0, 1.0], n)
    A = schwz.Csr(*_diag_csr(np.full(n, 2.0)))
    gm = schwz.Gmres(A, 0, 1, 4)
    d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
    it, rn = gm.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 5)
    assert it == 1 and rn == 0.0
    assert np.array_equal(d_x.cpu().numpy(), b / 2)


def test_gmres_near_breakdown_keeps_a_small_true_residual(schwz, torch_cuda):
    """Three distinct eigenvalues: the Krylov space is exhausted after three vectors and hn of the third is
    rounding noise, not zero.  The vectors after that are noise in any implementation, so no iterate parity
    here; what must hold is that the noise does no harm: a finite x whose true residual (longdouble) is at
    rounding level.  1e-12 |b|: some thousand u for a backward-stable solve of a system of condition 16."""
    torch = torch_cuda
    n = 3000
    rng = np.random.default_rng(6)
    d = rng.choice([1.0, 4.0, 16.0], n)
    b = rng.standard_normal(n)
    A = schwz.Csr(*_diag_csr(d))
    gm = schwz.Gmres(A, 0, 1, 8)
    d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
    it, rn = gm.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 8)
    x = d_x.cpu().numpy()
    assert it == 8 and np.isfinite(x).all() and np.isfinite(rn)
    res = b.astype(LD) - d.astype(LD) * x.astype(LD)
    rel = float(np.sqrt(np.dot(res, res)) / np.sqrt(np.dot(b.astype(LD), b.astype(LD))))
    print("near breakdown: true residual %.2e |b|, reported %.2e" % (rel, rn))
    assert rel <= 1e-12


def _small_nonsym(n, rng):
    import scipy.sparse as sp
    a = sp.diags([rng.uniform(-1, 0, max(n - 1, 0)), rng.uniform(3, 4, n), rng.uniform(-2, -1, max(n - 1, 0))],
                 [-1, 0, 1], shape=(n, n), format="csr")
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def test_gmres_restart_larger_than_n(schwz, oracle, torch_cuda):
    rng = np.random.default_rng(3)
    rp, col, val = _small_nonsym(5, rng)
    b, x0 = _rhs(5, 4)
    c = Case(schwz, oracle, torch_cuda, rp, col, val, 0, 1, 30, "n5/r30")
    for iters in (1, 3, 5):
        c.check_fixed(b, x0, iters)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_gmres_sizes_around_one_workgroup(schwz, oracle, torch_cuda, n):
    rng = np.random.default_rng(n)
    rp, col, val = _small_nonsym(n, rng)
    b, x0 = _rhs(n, n + 1)
    for pc in ("none", "jacobi"):
        c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], 4, "n%d/%s/r4" % (n, pc))
        for iters in sorted({1, min(n, 5), min(n, 9)}):
            c.check_fixed(b, x0, iters)


def test_gmres_max_iters_zero_leaves_x_alone(schwz, torch_cuda, convdiff):
    torch = torch_cuda
    rp, col, val = convdiff(12)
    n = len(rp) - 1
    b, x0 = _rhs(n)
    gm = schwz.Gmres(schwz.Csr(rp, col, val), 1, 1, 4)
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    it, rn = gm.solve(d_b.data_ptr(), d_x.data_ptr(), 1e-8, 0)
    assert it == 0
    assert np.array_equal(d_x.cpu().numpy(), x0)
    r = b.astype(LD) - hp.spmv(rp, col, val, x0)
    assert abs(rn - float(np.sqrt(np.dot(r, r)))) <= 64 * 2.0 ** -52 * rn


def test_gmres_start_vector_is_the_solution(schwz, torch_cuda):
    """Small integer data: b = A x0 holds exactly in float64 in any order, so beta == 0.0 and nothing runs."""
    torch = torch_cuda
    import scipy.sparse as sp
    n = 1000
    rng = np.random.default_rng(10)
    a = sp.diags([rng.integers(-3, 4, n - 1), rng.integers(5, 9, n), rng.integers(-3, 4, n - 1)], [-1, 0, 1],
                 shape=(n, n), format="csr").astype(np.float64)
    x0 = rng.integers(-8, 9, n).astype(np.float64)
    b = a @ x0
    gm = schwz.Gmres(schwz.Csr(a.indptr, a.indices, a.data), 0, 1, 4)
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    it, rn = gm.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 20)
    assert it == 0 and rn == 0.0
    assert np.array_equal(d_x.cpu().numpy(), x0)


# ---- a tolerance stop on and around the last vector of a cycle ---------------------------------------------------

@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_gmres_tolerance_stop_at_a_cycle_boundary(schwz, oracle, torch_cuda, convdiff, offset):
    """rtol is chosen from the reference's residual history so that the stop falls on vector 3 * restart
    (offset 0: the last vector of the third cycle), one before, one after.  The host reads the state one cycle
    behind, so with room left it launches one more cycle, which must change nothing: the same bits as a run
    whose max_iters ends at the stop."""
    restart, cyc = 4, 3
    rp, col, val = convdiff(40)
    n = len(rp) - 1
    b, _ = _rhs(n)
    c = Case(schwz, oracle, torch_cuda, rp, col, val, 1, 1, restart, "boundary%+d" % offset)
    target = cyc * restart + offset
    _, h = c.reference(b, None, target + 2)
    assert float(h[target]) < (1 - 1e-6) * float(h[target - 1]), "no clear gap in the reference's history"
    rtol = float(np.sqrt(h[target] * h[target - 1]) / h[0])
    x_ld, h_ld = c.reference(b, None, 4000, rtol)
    x_64, h_64 = c.reference(b, None, 4000, rtol, dtype=np.float64)
    assert len(h_ld) - 1 == len(h_64) - 1 == target
    x_long, it_long, rn_long = c.device(b, None, rtol, 4000)
    x_short, it_short, rn_short = c.device(b, None, rtol, target)
    assert it_long == it_short == target
    assert np.array_equal(x_long, x_short)
    assert rn_long == rn_short
    c.compare(x_long, rn_long, x_ld, h_ld, x_64, h_64, target)


# ---- reuse ------------------------------------------------------------------------------------------------------------

def test_gmres_second_solve_on_one_object(schwz, oracle, torch_cuda, convdiff):
    """H is zeroed at creation only: a solve that built 23 columns must leave nothing behind that a later,
    shorter solve reads."""
    rp, col, val = convdiff(40)
    n = len(rp) - 1
    b1, x1 = _rhs(n, 1)
    b2, x2 = _rhs(n, 2)
    c = Case(schwz, oracle, torch_cuda, rp, col, val, 2, 8, 30, "reuse")
    c.device(b1, x1, 0.0, 23)
    got, it, rn = c.device(b2, x2, 0.0, 5)
    fresh = schwz.Gmres(c.A, 2, 8, 30)
    exp, it_f, rn_f = c.device(b2, x2, 0.0, 5, gm=fresh)
    assert it == it_f == 5 and rn == rn_f
    assert np.array_equal(got, exp)
