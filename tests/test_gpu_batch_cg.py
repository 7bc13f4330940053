"""Block vectors (csrc/batch.hip): Csr.spmm, BatchCg.residual and the block CG, K = 2, 4, 8 columns stored
row-interleaved, against the extended-precision restatements of tests/hp_reference.py.

The CG tolerance is the rule of tests/test_gpu_chebyshev.py, unchanged, applied per column: hp.pcg runs twice, in
longdouble and (the same text) in float64, dev = |x_f64 - x_ld|_inf / |x_ld|_inf is the size of legitimate float64
rounding, and the device column must stay within 32 * max(dev, iters * 2^-52) of the longdouble iterate, likewise its
residual norm.  The reference decides the tolerance; the kernel's output never does.  Every case runs without a
preconditioner and with Jacobi, from a warm start X_0 != 0.  The references of a matrix are computed once for eight
columns and shared by the three widths: K = 2 and K = 4 take the first columns of the same data.

One exception, written down where it applies (_check_column): once the iteration count reaches the dimension of the
matrix, the exact residual is zero and what each of the three computations holds is its own rounding noise; there the
residual norm is held to an absolute bound derived from the condition number instead of a relative one."""
import numpy as np
import pytest

import hp_reference as hp
import stream_rig as rig
from test_gpu_chebyshev import lap1d_shifted, spd_band

pytestmark = pytest.mark.gpu

LD = np.longdouble
MARGIN = 32.0
PC = {"none": 0, "jacobi": 1}
BOTH = pytest.mark.parametrize("pc", ["none", "jacobi"])
WIDTHS = pytest.mark.parametrize("K", [2, 4, 8])
NCOL = 8


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _inf(a):
    return float(np.abs(a).max()) if len(a) else 0.0


def _columns(n, seed=29, scales=None):
    """Eight right-hand sides and warm starts, column j seeded by (seed, j); scales: powers of two per column."""
    B = np.empty((n, NCOL))
    X0 = np.empty((n, NCOL))
    for j in range(NCOL):
        rng = np.random.default_rng([seed, j])
        s = 1.0 if scales is None else scales[j]
        B[:, j] = rng.standard_normal(n) * s
        X0[:, j] = rng.standard_normal(n) * 0.1 * s
    return B, X0


_matrices = {}


class Matrix:
    """A matrix on the device with its block solvers, and the per-column references on the host (computed once)."""

    def __init__(self, schwz, torch, tag, rp, col, val):
        self.schwz, self.torch, self.tag = schwz, torch, tag
        self.rp, self.col, self.val = rp, col, val
        self.n = len(rp) - 1
        self.A = schwz.Csr(rp, col, val)
        self.solvers, self.refs = {}, {}

    def solver(self, pc, K):
        if (pc, K) not in self.solvers:
            self.solvers[pc, K] = self.schwz.BatchCg(self.A, PC[pc], K)
        return self.solvers[pc, K]

    def precond(self, pc, dtype):
        return hp.precond_jacobi(self.rp, self.col, self.val, dtype) if pc == "jacobi" else hp.precond_none(dtype)

    def reference(self, key, pc, b, x0, iters, rtol=0.0, keep=()):
        """{dtype: (x, hist, kept)} of one column; `key` names the column's data."""
        k = (key, pc, iters, rtol, tuple(keep))
        if k not in self.refs:
            hp.require_extended_precision()
            out = {}
            for dt in (LD, np.float64):
                kept = {m: None for m in keep}
                x, h = hp.pcg(self.rp, self.col, self.val, b, x0, self.precond(pc, dt), iters, rtol, dt, kept)
                out[dt] = (x, h, kept)
            self.refs[k] = out
        return self.refs[k]

    def device(self, pc, K, B, X0, rtol, max_iters, frozen=0, want_stats=True):
        d_b, d_x = _dev(self.torch, B[:, :K]), _dev(self.torch, X0[:, :K])
        s = self.solver(pc, K)
        it, rn = s.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, max_iters, frozen=frozen, want_stats=want_stats)
        self.torch.cuda.synchronize()
        if want_stats:
            assert s.last_stats() == (it, rn)
        return d_x.cpu().numpy().reshape(self.n, K), it, rn


def matrix(schwz, torch, tag, build):
    if tag not in _matrices:
        _matrices[tag] = Matrix(schwz, torch, tag, *build())
    return _matrices[tag]


def _check_column(tag, got, rn, x_ld, h_ld, x_64, h_64, iters, noise_bound=None):
    """The rule of test_gpu_chebyshev.Case.compare on one column.  noise_bound: the iteration count has reached the
    dimension of the matrix, so the exact residual is zero; the residual norm is then held to that absolute bound."""
    floor = max(iters, 1) * 2.0 ** -52
    scale = _inf(x_ld)
    dev_x = max(_inf(x_64.astype(LD) - x_ld) / scale, floor)
    err_x = _inf(got.astype(LD) - x_ld) / scale
    assert np.isfinite(got).all() and np.isfinite(rn)
    if noise_bound is None:
        r_ld = float(h_ld[-1])
        dev_r = max(abs(float(h_64[-1]) - r_ld) / r_ld, floor)
        err_r = abs(rn - r_ld) / r_ld
        print("%s iters %d: x err %.2e = %.2f dev (dev %.2e), resn err %.2e = %.2f dev" %
              (tag, iters, err_x, err_x / dev_x, dev_x, err_r, err_r / dev_r))
        assert err_r <= MARGIN * dev_r, (tag, iters, err_r, dev_r)
    else:
        print("%s iters %d: x err %.2e = %.2f dev (dev %.2e), resn %.2e against the noise bound %.2e" %
              (tag, iters, err_x, err_x / dev_x, dev_x, rn, noise_bound))
        assert rn <= noise_bound, (tag, iters, rn, noise_bound)
    assert err_x <= MARGIN * dev_x, (tag, iters, err_x, dev_x)


def _check_fixed(M, pc, K, B, X0, iters, key):
    got, it, rn = M.device(pc, K, B, X0, 0.0, iters)
    assert it == [iters] * K, (M.tag, pc, K, it)
    for j in range(K):
        ref = M.reference((key, j), pc, B[:, j], X0[:, j], iters)
        assert len(ref[LD][1]) - 1 == len(ref[np.float64][1]) - 1 == iters
        _check_column("%s/%s K=%d col %d" % (M.tag, pc, K, j), got[:, j], rn[j], ref[LD][0], ref[LD][1],
                      ref[np.float64][0], ref[np.float64][1], iters)
    return got


# ---- 1. the smallest shapes ------------------------------------------------------------------------------------------

@WIDTHS
@BOTH
@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 256, 257, 513])
def test_smallest_shapes(schwz, torch_cuda, n, pc, K):
    """The tails and both sides of the 256-row tile and of the 256 / K rows of a pass; zero iterations leave X
    bit-identical.  The matrix is tridiag(-1, 2.1, -1), condition number below 4.1 / 0.1 = 41.  For m >= n the Krylov
    space is exhausted: the exact residual is zero, a computed one is rounding noise of size m * 2^-53 * 41 * |r_0| at
    the most (the backward error of m updates, amplified by the condition number at the most), and a column may
    freeze on an exactly zero residual; the norm is held to 32 times that, the count to [n, m]."""
    M = matrix(schwz, torch_cuda, "lap1d_%d" % n, lambda: lap1d_shifted(n))
    B, X0 = _columns(n)
    got, it, rn = M.device(pc, K, B, X0, 0.0, 0)
    assert it == [0] * K and rig.same(got, X0[:, :K])
    for j in range(K):
        r0 = B[:, j].astype(LD) - hp.spmv(M.rp, M.col, M.val, X0[:, j])
        assert abs(rn[j] - float(np.sqrt(np.dot(r0, r0)))) <= 64 * 2.0 ** -52 * rn[j]
    for m in (1, 2, 9):
        got, it, rn = M.device(pc, K, B, X0, 0.0, m)
        for j in range(K):
            keep = (min(m, n),)
            ref = M.reference(("rhs29", j), pc, B[:, j], X0[:, j], min(m, n), keep=keep)
            x_ld, h_ld = ref[LD][2][min(m, n)], ref[LD][1]
            x_64, h_64 = ref[np.float64][2][min(m, n)], ref[np.float64][1]
            tag = "lap1d_%d/%s K=%d col %d" % (n, pc, K, j)
            if m < n:
                assert it[j] == m, (tag, it)
                _check_column(tag, got[:, j], rn[j], x_ld, h_ld, x_64, h_64, m)
            else:
                assert n <= it[j] <= m, (tag, it)
                noise = MARGIN * m * 2.0 ** -53 * 41.0 * float(h_ld[0])
                _check_column(tag, got[:, j], rn[j], x_ld, h_ld, x_64, h_64, m, noise_bound=noise)


# ---- 2. / 3. nonzero-limited tiles, the fallback of long rows, scaled columns ------------------------------------------

def _band31():
    rp, col, val = spd_band(700, 15, 31, wrap=True)
    assert np.diff(rp).min() == np.diff(rp).max() == 31 and np.diff(hp.tiles_of(rp)).max() == 66
    return rp, col, val


def _arrow():
    rp, col, val = hp.arrow_matrix(200, np.random.default_rng(200))
    assert np.diff(rp).max() == 200
    return rp, col, val


@WIDTHS
@BOTH
def test_nonzero_limited_tiles(schwz, torch_cuda, pc, K):
    """31 entries in every row: 66 rows fill a tile, most lanes of the last pass own no row and must store nothing;
    the tiles start at multiples of 2046 entries, so every second one is two entries into its aligned window."""
    M = matrix(schwz, torch_cuda, "band31", _band31)
    B, X0 = _columns(700)
    _check_fixed(M, pc, K, B, X0, 12, "rhs29")


@WIDTHS
@BOTH
def test_a_row_past_the_cap(schwz, torch_cuda, pc, K):
    """Row 0 holds 200 entries, past the 32-entry cap of the single-vector tile pipeline (the matrix is on that
    pipeline's fallback); the block kernels sum a row of any length that fits the staged window."""
    M = matrix(schwz, torch_cuda, "arrow200", _arrow)
    assert hp.stream_cap(M.rp) == 0
    B, X0 = _columns(200)
    _check_fixed(M, pc, K, B, X0, 12, "rhs29")


@WIDTHS
@BOTH
def test_scaled_columns(schwz, torch_cuda, pc, K):
    """Columns scaled by 2^20 and 2^-20 beside unscaled ones: a scalar shared across columns (alpha, beta, a partial
    sum in the wrong slot) shows at once."""
    M = matrix(schwz, torch_cuda, "band31", _band31)
    scales = [2.0 ** 20, 1.0, 2.0 ** -20, 1.0, 2.0 ** -20, 2.0 ** 20, 1.0, 2.0 ** 20]
    B, X0 = _columns(700, seed=31, scales=scales)
    _check_fixed(M, pc, K, B, X0, 9, "scaled31")


# ---- 4. tolerance stops, frozen columns, zero columns ----------------------------------------------------------------

def _stop_columns(n):
    """Columns whose start residual lies in 2, 4, 7, 11, 16 and 22 eigenvectors of tridiag(-1, 2.1, -1) (in exact
    arithmetic CG ends after that many steps, whatever the preconditioner: the diagonal is constant; in float64 the
    residual falls to about 1e-8 of its start there, and to 1e-8 itself after 2, 4, 9, 14, 18 and 22 steps), a zero
    column and a random one."""
    i = np.arange(1, n + 1)
    rng = np.random.default_rng(41)
    rp, col, val = lap1d_shifted(n)
    B, X0 = np.zeros((n, NCOL)), np.zeros((n, NCOL))
    for j, m in enumerate((2, 4, 7, 11, 16, 22)):
        v = sum(rng.uniform(0.5, 1.5) * np.sin(np.pi * (3 + 11 * q) * i / (n + 1)) for q in range(m))
        X0[:, j] = rng.standard_normal(n) * 0.1
        B[:, j] = np.asarray(hp.spmv(rp, col, val, X0[:, j] + v), dtype=np.float64)
    X0[:, 7] = rng.standard_normal(n) * 0.1
    B[:, 7] = rng.standard_normal(n)
    return B, X0


@WIDTHS
@BOTH
def test_columns_stop_at_their_own_iterations(schwz, torch_cuda, pc, K):
    """rtol = 1e-8, 30 iterations at the most.  The counts come from the float64 reference; before the device is
    asked, the test asserts that both references agree on them and that no residual norm of either lies within 5 % of
    the threshold: the longdouble and the float64 norms of these runs agree to far better than that, and so does any
    float64 summation order, so the rounding of a reduction cannot move a stop.  The random column runs out of
    iterations; the zero column never starts.  A second solve with more iterations leaves every column that had
    stopped bit-identical."""
    n, rtol, cap = 257, 1e-8, 30
    M = matrix(schwz, torch_cuda, "lap1d_257", lambda: lap1d_shifted(n))
    B, X0 = _stop_columns(n)
    want = []
    for j in range(K):
        if not B[:, j].any() and not X0[:, j].any():
            want.append(0)
            continue
        ref = M.reference(("stop41", j), pc, B[:, j], X0[:, j], cap, rtol=rtol)
        counts = {dt: len(ref[dt][1]) - 1 for dt in ref}
        assert counts[LD] == counts[np.float64], (j, counts)
        for dt in ref:
            h = np.asarray(ref[dt][1], dtype=np.float64)
            ratio = h / (rtol * h[0])
            assert not ((ratio > 1 / 1.05) & (ratio < 1.05)).any(), (j, ratio)
        want.append(counts[np.float64])
    assert len(set(want)) == len(want), want      # every column stops at an iteration of its own
    got, it, rn = M.device(pc, K, B, X0, rtol, cap)
    assert it == want, (it, want)
    for j in range(K):
        if want[j] == 0:
            assert rig.same(got[:, j], X0[:, j]) and rn[j] == 0.0
            continue
        ref = M.reference(("stop41", j), pc, B[:, j], X0[:, j], cap, rtol=rtol)
        _check_column("stop/%s K=%d col %d" % (pc, K, j), got[:, j], rn[j], ref[LD][0], ref[LD][1],
                      ref[np.float64][0], ref[np.float64][1], want[j])
    # the columns that stopped before iteration 12 hold the same bits after 12 iterations as after 30
    early, it12, _ = M.device(pc, K, B, X0, rtol, 12)
    for j in range(K):
        if want[j] < 12:
            assert it12[j] == want[j] and rig.same(early[:, j], got[:, j]), j
        else:
            assert it12[j] == 12


@WIDTHS
@BOTH
def test_zero_column_and_frozen_mask(schwz, torch_cuda, pc, K):
    """A zero column (b = 0, x_0 = 0) stays exactly zero and finite; a column named by the `frozen` mask keeps the
    bits of its X_0, counts no update, and the other columns hold the bits of the run without the mask."""
    M = matrix(schwz, torch_cuda, "band31", _band31)
    B, X0 = _columns(700)
    B, X0 = B.copy(), X0.copy()
    B[:, 1] = 0.0
    X0[:, 1] = 0.0
    free, it_free, _ = M.device(pc, K, B, X0, 0.0, 7)
    assert not free[:, 1].any() and it_free[1] == 0 and it_free[0] == 7
    mask = 1 << (K - 1)
    got, it, rn = M.device(pc, K, B, X0, 0.0, 7, frozen=mask)
    assert rig.same(got[:, K - 1], X0[:, K - 1]) and it[K - 1] == 0 and np.isfinite(rn).all()
    for j in range(K - 1):
        assert rig.same(got[:, j], free[:, j]) and it[j] == it_free[j]
    with pytest.raises(schwz.SchwzError) as e:
        M.device(pc, K, B, X0, 0.0, 1, frozen=1 << K)
    assert e.value.code == schwz.capi.ERR_INVALID


# ---- 5. independence of the columns, bit for bit -----------------------------------------------------------------------

@WIDTHS
@BOTH
def test_columns_are_independent(schwz, torch_cuda, pc, K):
    M = matrix(schwz, torch_cuda, "band31", _band31)
    B, X0 = _columns(700)
    base, it, rn = M.device(pc, K, B, X0, 0.0, 9)
    perm = np.roll(np.arange(K), 1)
    got, it_p, rn_p = M.device(pc, K, B[:, :K][:, perm], X0[:, :K][:, perm], 0.0, 9)
    assert rig.same(got, np.ascontiguousarray(base[:, perm])) and rn_p == [rn[p] for p in perm]
    # other data in every column but the first, a tolerance that lets the others stop on their own
    B2, X2 = _columns(700, seed=77, scales=[1.0, 2.0 ** 20, 2.0 ** -20, 1.0, 3.0, 1.0, 1.0, 1.0])
    B2[:, 0], X2[:, 0] = B[:, 0], X0[:, 0]
    B2[:, 1] = 0.0
    got, it2, rn2 = M.device(pc, K, B2, X2, 0.0, 9)
    assert rig.same(got[:, 0], base[:, 0]) and rn2[0] == rn[0] and it2[0] == 9


@BOTH
@pytest.mark.parametrize("tag,build,n", [("band31", _band31, 700), ("lap1d_513", lambda: lap1d_shifted(513), 513)])
def test_a_column_does_not_depend_on_the_width_of_its_block(schwz, torch_cuda, pc, tag, build, n):
    """The first two columns in blocks of 2, 4 and 8: the same bits, iterate, residual norm and residual sums -- every
    sum over rows runs in an order that does not depend on K (what lets solve_many pad its last block)."""
    torch = torch_cuda
    M = matrix(schwz, torch, tag, build)
    B, X0 = _columns(n)
    runs = {}
    for K in (2, 4, 8):
        got, it, rn = M.device(pc, K, B, X0, 0.0, 9)
        d_b, d_x = _dev(torch, B[:, :K]), _dev(torch, got)
        runs[K] = (got[:, :2].copy(), rn[:2], M.solver(pc, K).residual(d_b.data_ptr(), d_x.data_ptr())[:2])
    for K in (4, 8):
        assert rig.same(runs[K][0], runs[2][0]) and runs[K][1] == runs[2][1] and runs[K][2] == runs[2][2], K


# ---- 6. spmm and the residual forms, row by row ------------------------------------------------------------------------

_spmm = {}


def _spmm_case(name):
    """hp.rowsum_case with eight columns: column 0 is the case's own x and y0, the others are seeded draws, y0 scaled
    by exact powers of two so that it keeps the size of its row."""
    if name not in _spmm:
        hp.require_extended_precision()
        c = hp.rowsum_case(name)
        n, ncols = len(c["rp"]) - 1, c["ncols"]
        X, Y0 = np.empty((ncols, NCOL)), np.empty((n, NCOL))
        for j in range(NCOL):
            rng = np.random.default_rng([sum(name.encode()), j])
            X[:, j] = c["x"] if j == 0 else rng.standard_normal(ncols) * 2.0 ** (10 * (j % 3 - 1))
            Y0[:, j] = c["y0"] * 2.0 ** (j - 3) * (1.0 if j % 2 == 0 else -1.0)
        c["X"], c["Y0"], c["ref"] = X, Y0, {}
        _spmm[name] = c
    return _spmm[name]


def _worst(got, ref, bound):
    err = np.abs(got.astype(LD) - ref)
    assert (err[bound == 0] == 0).all()
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


@WIDTHS
@pytest.mark.parametrize("name", hp.ROWSUM_CASES)
def test_spmm_rows_meet_the_bound(schwz, torch_cuda, name, K):
    """Y = alpha A X + beta Y per column against hp.axpby at hp.axpby_bound, R = B - A X and the norm-only form
    against hp.residual at hp.residual_bound / hp.norm_sq_bound, on the matrices of the single-vector row-sum tests:
    rows of 5000 entries (tiles that do not fit the staged window), tiles two entries into their window, rectangular
    shapes, badly scaled rows, an empty row.  beta = 0 does not read Y (it holds NaN)."""
    torch = torch_cuda
    c = _spmm_case(name)
    a = (c["rp"], c["col"], c["val"])
    n, ncols = len(c["rp"]) - 1, c["ncols"]
    A = schwz.Csr(*a, ncols=ncols)
    d_x = _dev(torch, c["X"][:, :K])
    for alpha, beta in hp.ALPHA_BETA:
        y0 = c["Y0"][:, :K] if beta != 0 else np.full((n, K), np.nan)
        d_y = _dev(torch, y0)
        A.spmm(d_x.data_ptr(), d_y.data_ptr(), K, alpha, beta)
        torch.cuda.synchronize()
        got = d_y.cpu().numpy().reshape(n, K)
        for j in range(K):
            key = ("axpby", j, alpha, beta)
            if key not in c["ref"]:
                c["ref"][key] = (hp.axpby(*a, c["X"][:, j], alpha, beta, c["Y0"][:, j]),
                                 hp.axpby_bound(*a, c["X"][:, j], alpha, beta, c["Y0"][:, j]))
            ref, bound = c["ref"][key]
            w = _worst(got[:, j], ref, bound)
            print("%s K=%d col %d alpha %g beta %g: worst row at %.3f of its bound" % (name, K, j, alpha, beta, w))
            assert w <= 1.0, (name, K, j, alpha, beta, w)
    if n != ncols:
        return
    s = schwz.BatchCg(A, 0, K)
    d_b, d_r = _dev(torch, c["Y0"][:, :K]), _dev(torch, np.full((n, K), np.nan))
    nsq = s.residual(d_b.data_ptr(), d_x.data_ptr(), d_r.data_ptr())
    nsq_only = s.residual(d_b.data_ptr(), d_x.data_ptr())
    assert nsq == nsq_only
    got = d_r.cpu().numpy().reshape(n, K)
    for j in range(K):
        key = ("resid", j)
        if key not in c["ref"]:
            c["ref"][key] = (hp.residual(*a, c["X"][:, j], c["Y0"][:, j]), hp.residual_bound(*a, c["X"][:, j], c["Y0"][:, j]))
        ref, bound = c["ref"][key]
        w = _worst(got[:, j], ref, bound)
        nb = hp.norm_sq_bound(ref, bound, n)
        ne = abs(LD(nsq[j]) - np.sum(ref * ref))
        print("%s K=%d col %d residual: worst row at %.3f of its bound, norm^2 at %.3f" % (name, K, j, w, float(ne / nb)))
        assert w <= 1.0 and ne <= nb, (name, K, j, w, float(ne), float(nb))


def test_widths_other_than_2_4_8_are_refused(schwz, torch_cuda):
    rp, col, val = lap1d_shifted(5)
    A = schwz.Csr(rp, col, val)
    d = _dev(torch_cuda, np.zeros(5 * 8))
    for k in (0, 1, 3, 5, 16, -2):
        with pytest.raises(schwz.SchwzError) as e:
            A.spmm(d.data_ptr(), d.data_ptr(), k)
        assert e.value.code == schwz.capi.ERR_INVALID
        with pytest.raises(schwz.SchwzError) as e:
            schwz.BatchCg(A, 0, k)
        assert e.value.code == schwz.capi.ERR_INVALID
    with pytest.raises(schwz.NotImplementedSchwz):
        schwz.BatchCg(A, schwz.capi.PRECOND_ILU, 4)


# ---- 7. a non-default stream -------------------------------------------------------------------------------------------

def test_solve_and_spmm_on_a_stream(schwz, torch_cuda):
    """A fixed-work solve and an spmm enqueued whole on a non-blocking stream that a delay holds shut, inputs poisoned
    until the gate has passed (stream_rig.py), then a tolerance solve and the calls that read back; bit for bit the
    default-stream run."""
    torch = torch_cuda
    rp, col, val = _band31()
    K, n = 4, 700
    B, X0 = _columns(n)

    def body(r):
        A = r.hold(schwz.Csr(rp, col, val))
        s = r.hold(schwz.BatchCg(A, 1, K))
        d_b, d_x, d_x2 = r.input(B[:, :K].ravel()), r.input(X0[:, :K].ravel()), r.input(X0[:, :K].ravel())
        d_y = r.output(n * K)
        r.arm()
        r.call(s.solve, d_b.data_ptr(), d_x.data_ptr(), 0.0, 9, stream=r.handle, want_stats=False)
        r.call(A.spmm, d_x.data_ptr(), d_y.data_ptr(), K, 0.5, 0.0, stream=r.handle)
        r.snap(d_x)
        r.snap(d_y)
        r.check_shut("a fixed-work block solve and an spmm, enqueued whole")
        host = [r.call(s.last_stats, reads_back=True)]
        host.append(r.call(s.solve, d_b.data_ptr(), d_x2.data_ptr(), 1e-6, 40, stream=r.handle, reads_back=True))
        host.append(r.call(s.residual, d_b.data_ptr(), d_x2.data_ptr(), stream=r.handle, reads_back=True))
        r.snap(d_x2)
        return host
    snaps, host = rig.both(torch, body, "block CG and spmm")
    assert host[:K] == [9] * K and np.abs(snaps[1]).max() > 0
