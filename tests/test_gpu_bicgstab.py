"""Device-resident BiCGSTAB (csrc/bicgstab.hip) against the extended-precision restatement of hp_bicgstab.py: fixed
iteration counts from 4 workgroups to the grid-stride regime (a lane of the vector kernels holds one 16-byte element,
two rows: above 2048 * 256 elements = 1 048 576 rows the grid is capped, the kernels loop with two elements in flight
per lane and all 2048 partial sums of a dot product are in use; the odd last row has a lane of its own), matrices
stored in coded formats,
sizes around one workgroup, the branches (half-step stop, breakdown, zero start residual, max_iters = 0, reuse of
one object, tolerance stops at the top and at the half step around the host's polling batch), the solver inside a
RAS subdomain and a whole RAS run, and the C++ mirror.

Tolerance of the iterate comparisons: the rule of tests/test_gpu_gmres.py, unchanged.  Every case computes the
reference twice, in longdouble and (the same text) in float64, and takes dev = |x_f64 - x_ld|_inf / |x_ld|_inf as
the size of legitimate float64 rounding.  The kernel must stay within 32 * max(dev, iters * 2^-52) of the longdouble
iterate, and likewise for the residual norm.  The reference decides the tolerance; the kernel's output never does.
(A float64 run on the CPU that sums its dot products in the device's order -- per lane in sequence, a tree over the
workgroup, up to 2048 partial sums in sequence -- stays within 5.7 dev on convdiff(40) and convdiff(300) with the
default coefficients, with and without Jacobi, at 1 to 40 iterations: an emulation, not a device run.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hp_bicgstab
import hp_reference as hp

pytestmark = pytest.mark.gpu

LD = np.longdouble
MARGIN = 32.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPIEXEC = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
DRIVER = os.path.join(ROOT, "schwarz-lib_amd", "build", "bicgstab_driver")
PC = {"none": (0, 1), "jacobi": (1, 1), "bj8": (2, 8), "ilu": (3, 1)}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _inf(a):
    return float(np.abs(a).max()) if len(a) else 0.0


def _rhs(n, seed=29):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(n) * 0.1


class Case:
    """One matrix + preconditioner on the device, and both references on the host."""

    def __init__(self, schwz, oracle, torch, rp, col, val, precond, bs, tag, want_format=None):
        self.torch, self.rp, self.col, self.val = torch, rp, col, val
        self.n = len(rp) - 1
        self.tag = tag
        self.A = schwz.Csr(rp, col, val)
        if want_format is not None:
            assert self.A.format() == want_format, (tag, self.A.format())
        self.bi = schwz.Bicgstab(self.A, precond, bs)
        self.M = {dt: hp.make_precond(schwz, oracle, rp, col, val, precond, bs, dt) for dt in (LD, np.float64)}

    def device(self, b, x0, rtol, max_iters, bi=None):
        bi = bi or self.bi
        d_b = _dev(self.torch, b)
        d_x = _dev(self.torch, x0 if x0 is not None else np.zeros(self.n))
        it, rn = bi.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, max_iters)
        assert bi.last_stats() == (it, rn)
        return d_x.cpu().numpy(), it, rn

    def reference(self, b, x0, iters, rtol=0.0, dtype=LD):
        return hp_bicgstab.bicgstab(self.rp, self.col, self.val, b, x0, self.M[dtype], iters, rtol, dtype)

    def check_fixed(self, b, x0, iters):
        x_ld, h_ld, _, bd_ld = self.reference(b, x0, iters)
        x_64, h_64, _, bd_64 = self.reference(b, x0, iters, dtype=np.float64)
        assert bd_ld == bd_64 == 0 and len(h_ld) - 1 == len(h_64) - 1 == iters, self.tag
        got, it, rn = self.device(b, x0, 0.0, iters)
        assert it == iters and self.bi.breakdown() == 0, (self.tag, it)
        self.compare(got, rn, x_ld, h_ld, x_64, h_64, iters)

    def compare(self, got, rn, x_ld, h_ld, x_64, h_64, iters):
        floor = iters * 2.0 ** -52
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


# ---- fixed iteration counts ---------------------------------------------------------------------------------

@pytest.mark.parametrize("pc", ["none", "jacobi", "bj8", "ilu"])
def test_bicgstab_fixed_iterations_convdiff_40(schwz, oracle, torch_cuda, convdiff, pc):
    rp, col, val = convdiff(40)
    b, x0 = _rhs(len(rp) - 1)
    c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], "convdiff40/%s" % pc)
    for iters in (1, 5, 12, 23):
        c.check_fixed(b, x0, iters)


@pytest.mark.parametrize("pc", ["none", "jacobi", "bj8", "ilu"])
def test_bicgstab_fixed_iterations_on_600625_rows(schwz, oracle, torch_cuda, convdiff, pc):
    """n = 600 625, odd: 300 312 elements of 16 bytes on 1174 workgroups -- more rows than the 524 288 lanes of a
    capped grid, but with two rows per lane still one trip per lane (the kernels stride from 1 048 576 rows on: the
    next test) -- and the last row is the odd-tail lane's.  Every preconditioner at a size where their kernels are
    far past one workgroup."""
    rp, col, val = convdiff(775)
    n = len(rp) - 1
    assert n == 600625 and n > 2048 * 256 and n % 2 == 1
    b, x0 = _rhs(n)
    c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], "convdiff775/%s" % pc)
    c.check_fixed(b, x0, 5)


@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_bicgstab_fixed_iterations_past_the_grid_cap(schwz, oracle, torch_cuda, convdiff, pc):
    """n = 1 050 625, odd: 525 312 elements > 2048 * 256 = 524 288, so the grid is capped at kMaxGrid, nparts ==
    kMaxGrid, the host picks the kernels with two elements in flight per lane, the first 1024 lanes make a second
    trip (whose second element is past the end: the `i < n2` guards), and the odd tail goes with striding.  Three
    iterations: the 80-bit reference costs about a second per iteration here."""
    rp, col, val = convdiff(1025)
    n = len(rp) - 1
    assert n == 1050625 and (n >> 1) > 2048 * 256 and n % 2 == 1
    b, x0 = _rhs(n)
    c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], "convdiff1025/%s" % pc)
    c.check_fixed(b, x0, 3)


@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("coding", ["lap3d_pairs", "lap2d_dictionary"])
def test_bicgstab_fixed_iterations_on_coded_matrices(schwz, oracle, torch_cuda, monkeypatch, coding, pc):
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
    c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], "%s/%s" % (coding, pc), want_format=want)
    c.check_fixed(b, x0, 12)


def _small_nonsym(n, rng):
    import scipy.sparse as sp
    a = sp.diags([rng.uniform(-1, 0, max(n - 1, 0)), rng.uniform(3, 4, n), rng.uniform(-2, -1, max(n - 1, 0))],
                 [-1, 0, 1], shape=(n, n), format="csr")
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 512, 513, 514, 515])
def test_bicgstab_sizes_around_one_workgroup(schwz, oracle, torch_cuda, n):
    """The odd tail alone (n = 1), one lane (n = 2), and both sides of the boundaries: a lane holds one 16-byte
    element (two rows), so 256 rows fill half a workgroup and 512 rows a whole one; 513 rows launch a second
    workgroup that has no element (the tail is workgroup 0's), 514 rows give it one, 515 one and the tail."""
    rng = np.random.default_rng(n)
    rp, col, val = _small_nonsym(n, rng)
    b, x0 = _rhs(n, n + 1)
    for pc in ("none", "jacobi"):
        c = Case(schwz, oracle, torch_cuda, rp, col, val, *PC[pc], "n%d/%s" % (n, pc))
        if n == 1:
            # exact after the half step of iteration 0 in exact arithmetic; in floating point s may be a rounding
            # residue: whatever the references do, they must do alike, and the device like them
            x_ld, h_ld, _, bd = c.reference(b, x0, 1)
            got, it, rn = c.device(b, x0, 0.0, 1)
            assert it == len(h_ld) - 1 == 1 and np.isfinite(got).all()
            assert abs(got[0] - float(x_ld[0])) <= MARGIN * 2.0 ** -52 * abs(float(x_ld[0]))
            continue
        # (fewer iterations than rows: once the Krylov space is exhausted the recurrences carry rounding noise, for
        # which there is no reference)
        for iters in sorted({1, min(n - 1, 3), min(n - 1, 6)}):
            c.check_fixed(b, x0, iters)


# ---- branches -----------------------------------------------------------------------------------------------

def _diag_csr(d):
    n = len(d)
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(d, dtype=np.float64)


@pytest.mark.parametrize("n", [3, 4 ** 5 + 1])
def test_bicgstab_half_step_stop(schwz, torch_cuda, n):
    """A = 2 I, b = +-1 (n > 3: 1025 rows, 512 elements that fill two workgroups, a third one without any, and the odd tail): v = 2 r, sigma = 2 rho, alpha = 1/2
    and s = r - r / 2 - r / 2... every intermediate is a dyadic number float64 holds exactly in any summation
    order, so ||s|| == 0: the half step of iteration 0 ends the solve, iters = 1, x = b / 2 exactly."""
    torch = torch_cuda
    b = np.random.default_rng(1).choice([-1.0, 1.0], n)
    bi = schwz.Bicgstab(schwz.Csr(*_diag_csr(np.full(n, 2.0))), 0, 1)
    d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
    it, rn = bi.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 5)
    assert (it, rn) == (1, 0.0) and bi.breakdown() == 0
    assert np.array_equal(d_x.cpu().numpy(), b / 2)


def test_bicgstab_breakdown_on_the_skew_matrix(schwz, torch_cuda):
    """[[0, 1], [-1, 0]]: rhat.v = r.(A r) = r0 r1 - r1 r0 = 0 exactly (r_0 = (3.25, 4.5): the product is exact in
    float64, fused or not): breakdown 2 before x is touched.  An ordinary finite input whose solve ends with a
    flag."""
    torch = torch_cuda
    rp, col, val = np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, -1.0])
    b, x0 = np.array([3.0, 4.0]), np.array([0.5, -0.25])
    x_ref, h_ref, _, bd_ref = hp_bicgstab.bicgstab(rp, col, val, b, x0, hp.precond_none(np.float64), 5, 0.0,
                                                   np.float64)
    assert bd_ref == 2 and len(h_ref) == 1
    bi = schwz.Bicgstab(schwz.Csr(rp, col, val), 0, 1)
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    it, rn = bi.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 5)
    assert it == 0 and bi.breakdown() == 2
    # r_0 = (3.25, 4.5), ||r_0||^2 = 30.8125 exactly: the two square roots may differ by an ulp
    assert abs(rn - float(h_ref[0])) <= 2.0 ** -51 * float(h_ref[0])
    assert np.array_equal(d_x.cpu().numpy(), x0)
    # the flag belongs to the last solve: the next one on the same object clears it
    it, rn = bi.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 0)
    assert it == 0 and bi.breakdown() == 0
    assert np.array_equal(d_x.cpu().numpy(), x0)


def test_bicgstab_start_vector_is_the_solution(schwz, torch_cuda):
    """Small integer data: b = A x0 holds exactly in float64 in any order, so ||r_0|| == 0.0 and nothing runs."""
    torch = torch_cuda
    import scipy.sparse as sp
    n = 1000
    rng = np.random.default_rng(10)
    a = sp.diags([rng.integers(-3, 4, n - 1), rng.integers(5, 9, n), rng.integers(-3, 4, n - 1)], [-1, 0, 1],
                 shape=(n, n), format="csr").astype(np.float64)
    x0 = rng.integers(-8, 9, n).astype(np.float64)
    b = a @ x0
    bi = schwz.Bicgstab(schwz.Csr(a.indptr, a.indices, a.data), 1, 1)
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    it, rn = bi.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 20)
    assert it == 0 and rn == 0.0 and bi.breakdown() == 0
    assert np.array_equal(d_x.cpu().numpy(), x0)


def test_bicgstab_max_iters_zero_leaves_x_alone(schwz, torch_cuda, convdiff):
    torch = torch_cuda
    rp, col, val = convdiff(12)
    n = len(rp) - 1
    b, x0 = _rhs(n)
    bi = schwz.Bicgstab(schwz.Csr(rp, col, val), 1, 1)
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    it, rn = bi.solve(d_b.data_ptr(), d_x.data_ptr(), 1e-8, 0)
    assert it == 0 and bi.breakdown() == 0
    assert np.array_equal(d_x.cpu().numpy(), x0)          # bit-identical
    r = b.astype(LD) - hp.spmv(rp, col, val, x0)
    assert abs(rn - float(np.sqrt(np.dot(r, r)))) <= 64 * 2.0 ** -52 * rn


def test_bicgstab_second_solve_on_one_object(schwz, oracle, torch_cuda, convdiff):
    """A long solve, then a warm-started short one on the same object: the state is reset, nothing of the first
    solve is read -- the same bits as a fresh object gives -- and the result is the reference's."""
    rp, col, val = convdiff(40)
    n = len(rp) - 1
    b1, x1 = _rhs(n, 1)
    b2, _ = _rhs(n, 2)
    c = Case(schwz, oracle, torch_cuda, rp, col, val, 2, 8, "reuse")
    warm, _, _ = c.device(b1, x1, 0.0, 23)
    got, it, rn = c.device(b2, warm, 0.0, 5)
    fresh = schwz.Bicgstab(c.A, 2, 8)
    exp, it_f, rn_f = c.device(b2, warm, 0.0, 5, bi=fresh)
    assert it == it_f == 5 and rn == rn_f
    assert np.array_equal(got, exp)
    x_ld, h_ld, _, _ = c.reference(b2, warm, 5)
    x_64, h_64, _, _ = c.reference(b2, warm, 5, dtype=np.float64)
    c.compare(got, rn, x_ld, h_ld, x_64, h_64, 5)


# ---- tolerance stops around the host's polling batch ----------------------------------------------------------------

GAP = 1.2


# (half, k) -> seed of the right-hand side: the first seeds from 100 on whose float64 reference history on
# convdiff(40) with Jacobi has the gap at iteration k (a full-step norm below every earlier half-step norm is rare:
# hence the large seeds of the top stops)
STOP_SEEDS = {(False, 7): 117, (False, 8): 205, (False, 9): 609, (True, 7): 102, (True, 8): 112, (True, 9): 104}


def _find_stop(c, n, k, half):
    """A right-hand side and rtol for which the solve stops at the top of iteration k (half: in the middle of it):
    rtol * nu is the geometric mean of the norm that is to stop the solve and the smallest norm any earlier test
    saw, the two at least a factor GAP apart (rounding moves these norms by about 1e-13 relative)."""
    b, _ = _rhs(n, STOP_SEEDS[(half, k)])
    _, h, hh, bd = c.reference(b, None, k + 2)
    assert bd == 0 and len(h) - 1 >= k + 1
    h, hh = [float(v) for v in h], [float(v) for v in hh]
    # the tests in order: top 0, half 0, top 1, half 1, ...
    earlier = h[:k] + hh[:k] + ([h[k]] if half else [])
    hit = hh[k] if half else h[k]
    assert hit * GAP <= min(earlier), "no clear gap at iteration %d: take another seed" % k
    return b, float(np.sqrt(hit * min(earlier)) / h[0])


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_bicgstab_tolerance_stop_around_the_polling_batch(schwz, oracle, torch_cuda, convdiff, offset, half):
    """The host reads the state one batch behind the launches: a stop at the top (half: at the half step) of
    iteration batch - 1, batch, batch + 1 is followed by up to two batches of launches that must change nothing --
    the same bits as a run whose max_iters ends at the stop, and the iteration count of the reference."""
    batch = schwz.capi.BICGSTAB_POLL_BATCH
    rp, col, val = convdiff(40)
    n = len(rp) - 1
    c = Case(schwz, oracle, torch_cuda, rp, col, val, 1, 1, "stop%+d%s" % (offset, "/half" if half else ""))
    k = batch + offset
    b, rtol = _find_stop(c, n, k, half)
    want = k + 1 if half else k
    x_ld, h_ld, hh_ld, _ = c.reference(b, None, 4000, rtol)
    x_64, h_64, hh_64, _ = c.reference(b, None, 4000, rtol, dtype=np.float64)
    assert len(h_ld) - 1 == len(h_64) - 1 == want
    assert len(hh_ld) == len(hh_64) == (k + 1 if half else k)
    x_long, it_long, rn_long = c.device(b, None, rtol, 4000)
    x_short, it_short, rn_short = c.device(b, None, rtol, want)
    assert it_long == it_short == want and c.bi.breakdown() == 0
    assert np.array_equal(x_long, x_short)
    assert rn_long == rn_short
    c.compare(x_long, rn_long, x_ld, h_ld, x_64, h_64, want)


# ---- inside RAS -----------------------------------------------------------------------------------------------------

def _csr(rp, col, val):
    import scipy.sparse as sp
    n = len(rp) - 1
    return sp.csr_matrix((np.asarray(val, dtype=np.float64), np.asarray(col), np.asarray(rp)), shape=(n, n))


def _write_mtx(path, rp, col, val):
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, rp[-1]))
        for r, c, v in zip(rows, col, val):
            f.write("%d %d %.17g\n" % (r + 1, c + 1, v))
    return path


def _gmres_exact_reference(oracle, rp, col, val, P, m):
    """The oracle's RAS with GMRES local solves that are exact to rounding (Krylov space = the local system)."""
    N = len(rp) - 1
    return oracle.ras_run(rp, col, val, np.ones(N), P, np.asarray(m.first_row, dtype=np.int32),
                          oracle.make_settings(max_iters=m.max_iters, tol=m.tolerance, local_tol=1e-14,
                                               local_max_iters=N, non_symmetric=1, restart_iter=N))


@pytest.mark.parametrize("P", [1, 3])
def test_ras_with_bicgstab_local_solves(schwz, oracle, torch_cuda, convdiff, tmp_path, P):
    import scipy.sparse.linalg as sl
    rp, col, val = convdiff(30)
    n = len(rp) - 1
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    s = schwz.Settings(matrix_filename=path, explicit_laplacian=False, non_symmetric_matrix=True)
    m = schwz.Metadata(num_subdomains=P, non_symmetric_solver="bicgstab", local_precond="block-jacobi",
                       precond_max_block_size=1, local_solver_tolerance=1e-12, tolerance=1e-8, max_iters=400)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    assert all(sd.nonsym_solver() == schwz.capi.NONSYM_BICGSTAB for sd in solver.subdomains.values())
    out = solver.run()
    r = _gmres_exact_reference(oracle, rp, col, val, P, m)
    x = sl.spsolve(_csr(rp, col, val).tocsc(), np.ones(n))
    print("P = %d: %d outer iterations, oracle %d" % (P, out["iter_count"], r["iter_count"]))
    assert out["converged"] and r["converged"]
    assert abs(out["iter_count"] - r["iter_count"]) <= 1
    assert np.isfinite(out["solution"]).all()
    assert np.abs(out["solution"] - x).max() <= 1e-8 * np.abs(x).max()


def test_default_settings_keep_gmres(schwz, torch_cuda, convdiff, tmp_path):
    rp, col, val = convdiff(12)
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    s = schwz.Settings(matrix_filename=path, explicit_laplacian=False, non_symmetric_matrix=True, restart_iter=10)
    m = schwz.Metadata(num_subdomains=2, tolerance=1e-8, max_iters=50)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(2), quiet=True)
    solver.initialize()
    assert all(sd.nonsym_solver() == schwz.capi.NONSYM_GMRES for sd in solver.subdomains.values())


class _Handle:
    def __init__(self, h):
        self.h = h


def test_subdomain_step_is_the_standalone_solver(schwz, torch_cuda, convdiff):
    """One local solve of a subdomain with neighbours (overlap rows, a halo) is schwz_bicgstab_solve on the local
    matrix with b~ and the start vector y: the same bits.  The setter round-trips, refuses what it must, and the
    two-stage cap takes effect on the next solve."""
    torch, c = torch_cuda, schwz.capi
    rp, col, val = convdiff(30)
    P, me = 3, 1
    prob = schwz.Problem.from_csr(rp, col, val)
    sd = schwz.Subdomain(prob, P, me, 2, schwz.partition_regular(prob.N, P))
    nloc = sd.local_size_x
    rng = np.random.default_rng(5)
    sd.to_device(rng.standard_normal(nloc), precond=c.PRECOND_JACOBI, local_tol=0.0, local_max_iters=4,
                 non_symmetric=True, restart_iter=7)
    assert sd.nonsym_solver() == c.NONSYM_GMRES
    sd.set_nonsym_solver(c.NONSYM_BICGSTAB)
    assert sd.nonsym_solver() == c.NONSYM_BICGSTAB
    sd.set_nonsym_solver(c.NONSYM_GMRES)
    assert sd.nonsym_solver() == c.NONSYM_GMRES
    sd.set_nonsym_solver(c.NONSYM_BICGSTAB)
    sd.set_nonsym_solver(c.NONSYM_BICGSTAB)
    assert sd.nonsym_solver() == c.NONSYM_BICGSTAB
    with pytest.raises(schwz.SchwzError) as e:
        sd.set_nonsym_solver(2)
    assert e.value.code == c.ERR_INVALID
    with pytest.raises(schwz.NotImplementedSchwz):
        sd.set_local_precision(c.PRECISION_F32)
    assert (sd.early_pack_ok(), sd.cg_flavour(), sd.y_form()) == (0, 0, 0)

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

    put(0, rng.standard_normal(nx))
    put(2, rng.standard_normal(nloc) * 0.1)
    sd.update_boundary()
    torch.cuda.synchronize()
    bt, y0 = get(1), get(2)
    h = C.c_void_p()
    c.check(c.lib.schwz_ras_local_csr(sd.h, C.byref(h)))
    alone = schwz.Bicgstab(_Handle(h), c.PRECOND_JACOBI, 1)

    def standalone(iters):
        d_b, d_x = _dev(torch, bt), _dev(torch, y0)
        it, rn = alone.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, iters)
        return d_x.cpu().numpy(), it, rn

    assert sd.local_solve(want_iters=True) == 4
    torch.cuda.synchronize()
    exp, it, rn = standalone(4)
    assert it == 4
    assert np.array_equal(get(2), exp)
    assert sd.last_inner_stats() == (4, rn)
    # the two-stage cap, and a solve launched without asking for the count
    sd.set_local_max_iters(2)
    put(2, y0)
    sd.local_solve()
    torch.cuda.synchronize()
    exp2, it2, rn2 = standalone(2)
    assert np.array_equal(get(2), exp2)
    assert sd.last_inner_stats() == (2, rn2)
    assert not np.array_equal(exp, exp2)
    # a symmetric subdomain has no such choice
    sd2 = schwz.Subdomain(prob, P, me, 2, schwz.partition_regular(prob.N, P))
    sd2.to_device(np.ones(nloc), precond=c.PRECOND_JACOBI)
    with pytest.raises(schwz.NotImplementedSchwz):
        sd2.set_nonsym_solver(c.NONSYM_BICGSTAB)
    assert sd2.nonsym_solver() == c.NONSYM_GMRES


# ---- the C++ mirror -------------------------------------------------------------------------------------------------

def _driver(nranks, *args):
    if not os.path.exists(DRIVER):
        pytest.skip("bicgstab_driver not built (`make -C schwarz-lib_amd bicgstab_driver`, needs MPI)")
    if not os.path.exists(MPIEXEC):
        pytest.skip("no mpiexec on this machine")
    cmd = [MPIEXEC, "-n", str(nranks), DRIVER] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_mirror_runs_bicgstab_like_the_python_host(schwz, torch_cuda, convdiff, tmp_path):
    rp, col, val = convdiff(30)
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    P = 2
    p = _driver(P, "bicgstab", path, 1e-8, 400, 1)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "(BiCGSTAB)" in p.stdout and "restart iter" not in p.stdout
    res = re.search(r"RESULT iters=(\d+) solnorm=([0-9.eE+-]+)", p.stdout)
    final = re.search(r"^ residual norm ([0-9.eE+-]+)$", p.stdout, re.M)
    assert res and final, p.stdout
    s = schwz.Settings(matrix_filename=path, explicit_laplacian=False, non_symmetric_matrix=True, overlap=2)
    s.convergence_settings.enable_global_check = True
    m = schwz.Metadata(num_subdomains=P, non_symmetric_solver="bicgstab", local_precond="block-jacobi",
                       precond_max_block_size=1, local_solver_tolerance=1e-12, tolerance=1e-8, max_iters=400)
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


def test_mirror_refuses_an_unknown_solver_name(convdiff, tmp_path):
    rp, col, val = convdiff(6)
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    p = _driver(1, "cgs", path, 1e-8, 10, 1)
    assert p.returncode == 3, p.stdout + p.stderr
    assert "REFUSED" in p.stdout
