"""The extended-precision references of hp_reference.py, pinned on the CPU: against scipy, against the C
oracle, against a dense solve, and the componentwise substitution bound against a float64 run of the same
substitution (it must hold, and it must not be slack by orders of magnitude)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sl

import hp_reference as hp

LD = np.longdouble


def test_longdouble_is_extended_precision():
    hp.require_extended_precision()
    assert np.finfo(LD).eps < 2.0 ** -60


def _csr(f, name, n):
    return sp.csr_matrix((f[name + "_val"], f[name + "_col"], f[name + "_rp"]), shape=(n, n))


def test_spmv_matches_scipy(convdiff):
    rng = np.random.default_rng(3)
    rp, col, val = convdiff(23)
    n = len(rp) - 1
    x = rng.standard_normal(n)
    a = sp.csr_matrix((val, col, rp), shape=(n, n))
    exp = a @ x
    for dtype in (LD, np.float64):
        got = hp.spmv(rp, col, val, x, dtype)
        assert got.dtype == np.dtype(dtype)
        assert np.abs(got.astype(np.float64) - exp).max() <= 8 * 2.0 ** -52 * (abs(a) @ np.abs(x)).max()
    # ragged rows, an empty row, one long row
    m = sp.random(200, 200, density=0.03, random_state=5, format="lil")
    m[7, :] = rng.standard_normal(200)
    m[11, :] = 0
    m = m.tocsr()
    m.sort_indices()
    got = hp.spmv(m.indptr, m.indices, m.data, x[:200])
    assert np.abs(got.astype(np.float64) - m @ x[:200]).max() <= 256 * 2.0 ** -52 * (abs(m) @ np.abs(x[:200])).max()


def test_trs_apply_matches_spsolve():
    rng = np.random.default_rng(11)
    f = hp.five_point_factors(17 * 13, 17, rng)
    n = 17 * 13
    L, U = hp.factors(f)
    assert L.nlevels == 17 + 13 - 1 and U.nlevels == 17 + 13 - 1
    b = rng.standard_normal(n)
    p, q = rng.permutation(n), rng.permutation(n)
    a = (_csr(f, "l", n) @ _csr(f, "u", n)).tocsc()
    for pin, pout in ((None, None), (p, p), (p, q)):
        w = b if pin is None else b[pin]
        w0 = sl.spsolve(a, w)
        exp = w0.copy()
        if pout is not None:
            exp = np.zeros(n)
            exp[pout] = w0
        got = hp.trs_apply(L, U, pin, pout, b).astype(np.float64)
        assert np.abs(got - exp).max() <= 1e-11 * np.abs(exp).max()
    # the two substitutions alone, against scipy's
    x = hp.lower_solve(f["l_rp"], f["l_col"], f["l_val"], b).astype(np.float64)
    assert np.abs(x - sl.spsolve_triangular(_csr(f, "l", n), b, lower=True)).max() <= 1e-12 * np.abs(x).max()
    x = hp.upper_solve(f["u_rp"], f["u_col"], f["u_val"], b).astype(np.float64)
    assert np.abs(x - sl.spsolve_triangular(_csr(f, "u", n), b, lower=False)).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("pc", [(0, 1), (1, 1), (2, 8), (3, 1)])
@pytest.mark.parametrize("restart", [1, 4, 30])
def test_gmres_float64_matches_the_oracle(schwz, oracle, convdiff, restart, pc):
    """The same cases and the same tolerance as test_gmres_matches_oracle uses for the device solver."""
    precond, bs = pc
    rp, col, val = convdiff(40)
    n = len(rp) - 1
    rng = np.random.default_rng(29)
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n) * 0.1
    M = hp.make_precond(schwz, oracle, rp, col, val, precond, bs, np.float64)
    for iters in (1, 5, 23):
        exp, it_o, rn_o = oracle.gmres(rp, col, val, b, x0, precond, 0.0, iters, restart, bs)
        got, hist = hp.gmres(rp, col, val, b, x0, M, iters, restart, dtype=np.float64)
        assert len(hist) - 1 == it_o == iters
        assert np.abs(got - exp).max() <= 1e-9 * np.abs(exp).max()
        assert abs(hist[-1] - rn_o) <= 1e-8 * rn_o
    exp, it_o, rn_o = oracle.gmres(rp, col, val, b, None, precond, 1e-9, 4000, restart, bs)
    got, hist = hp.gmres(rp, col, val, b, None, M, 4000, restart, rtol=1e-9, dtype=np.float64)
    assert abs(len(hist) - 1 - it_o) <= max(1, restart // 8)
    assert np.abs(got - exp).max() <= 1e-6 * np.abs(exp).max()


def test_gmres_longdouble_is_a_direct_solve_once_the_krylov_space_is_full(convdiff):
    rng = np.random.default_rng(2)
    rp, col, val = convdiff(5)
    n = len(rp) - 1
    a = sp.csr_matrix((val, col, rp), shape=(n, n)).toarray()
    b = rng.standard_normal(n)
    exp = np.linalg.solve(a, b)
    for M in (hp.precond_none(), hp.precond_jacobi(rp, col, val),
              hp.precond_block_jacobi(rp, col, val, np.arange(0, n + 1, 5))):
        x, hist = hp.gmres(rp, col, val, b, None, M, n, n)
        assert len(hist) - 1 == n
        assert hist[-1] <= 1e-14 * hist[0]
        assert np.abs(x.astype(np.float64) - exp).max() <= 1e-12 * np.abs(exp).max()
        # the history is the true residual norm at every step of the first cycle
        x5, h5 = hp.gmres(rp, col, val, b, None, M, 5, n)
        true = np.linalg.norm((b - a @ x5.astype(np.float64)))
        assert abs(float(h5[-1]) - true) <= 1e-12 * float(h5[0])


def test_dense_inverse_and_block_jacobi():
    rng = np.random.default_rng(4)
    a = rng.standard_normal((7, 7)) + 4 * np.eye(7)
    inv = hp._dense_inverse(a.astype(LD))
    assert np.abs((inv @ a.astype(LD)) - np.eye(7)).max() <= 1e-17


@pytest.mark.parametrize("kind", ["ilu2d", "chain"])
def test_trs_error_bound_holds_and_is_tight(kind):
    """A float64 run of the same substitution stays inside the derived bound (max err / bound <= 1) and comes
    within a factor 16 of it: the bound neither fails on the reference's own account nor hides a
    wrong kernel behind orders of magnitude of slack."""
    rng = np.random.default_rng(8)
    if kind == "ilu2d":
        f, n = hp.five_point_factors(64 * 48, 64, rng), 64 * 48
    else:
        n = 4000
        f = hp.bidiagonal_factors(n, rng)
    L, U = hp.factors(f)
    b = rng.standard_normal(n)
    y, w1, w0 = hp.trs_apply(L, U, None, None, b, parts=True)
    bound = hp.trs_error_bound(L, U, w1, w0)
    y64 = hp.trs_apply(L, U, None, None, b, dtype=np.float64)
    assert y64.dtype == np.float64
    ratio = (np.abs(y64.astype(LD) - y) / bound).max()
    print("max err / bound (%s): %.3f" % (kind, ratio))
    assert ratio <= 1.0
    assert ratio >= 1.0 / 16


def test_jacobi_sweep_solve_matches_scipy_and_its_bound_holds():
    rng = np.random.default_rng(9)
    f = hp.five_point_factors(1200, 40, rng)
    n = 1200
    L, U = hp.factors(f)
    b = rng.standard_normal(n)
    for k in (1, 3):
        out = b
        for name in ("l", "u"):
            T = _csr(f, name, n)
            d = T.diagonal()
            Ts = T - sp.diags(d)
            x = out / d
            for _ in range(k):
                x = (out - Ts @ x) / d
            out = x
        y, bound = hp.jacobi_sweep_solve(L, U, b, k, bound=True)
        assert np.abs(y.astype(np.float64) - out).max() <= 1e-13 * np.abs(out).max()
        assert np.array_equal(y, hp.jacobi_sweep_solve(L, U, b, k))
        y64 = hp.jacobi_sweep_solve(L, U, b, k, dtype=np.float64)
        ratio = (np.abs(y64.astype(LD) - y) / bound).max()
        print("jacobi sweeps %d: max err / bound %.3f" % (k, ratio))
        assert ratio <= 1.0
    # enough sweeps make the series exact
    k = max(L.nlevels, U.nlevels) - 1
    y = hp.jacobi_sweep_solve(L, U, b, k)
    assert np.abs(y - hp.trs_apply(L, U, None, None, b)).max() <= 1e-17 * np.abs(y).max()


def test_parilu_restatement_reaches_ilu0(oracle):
    rp, col, val = oracle.laplacian2d(6)
    rp, col, val = np.asarray(rp, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64)
    pat = hp.Pattern(rp, col)
    lv, uv = hp.parilu_numpy(pat, val, pat.depth())
    f = oracle.ilu0(rp, col, val)
    assert np.array_equal(pat.l_col, f["l_col"]) and np.array_equal(pat.u_col, f["u_col"])
    assert np.abs(lv - f["l_val"]).max() <= 1e-14 and np.abs(uv - f["u_val"]).max() <= 1e-14


# ---- preconditioned CG, the slicing stencil, pairwise dot products ------------------------------------------------

@pytest.mark.parametrize("pc", [(0, 1), (1, 1), (2, 8), (3, 1)])
def test_pcg_float64_matches_the_oracle(schwz, oracle, pc):
    """Two float64 statements of one recurrence on a system of condition ~ 700: they differ by rounding only, so
    1e-11 (not the 1e-9 the device CG is held to against the oracle)."""
    precond, bs = pc
    rp, col, val = oracle.laplacian2d(40)
    n = len(rp) - 1
    rng = np.random.default_rng(29)
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n) * 0.1
    M = hp.make_precond(schwz, oracle, rp, col, val, precond, bs, np.float64)
    keep = {1: None, 5: None, 23: None}
    got, hist = hp.pcg(rp, col, val, b, x0, M, 23, dtype=np.float64, keep=keep)
    assert got.dtype == np.float64 and np.array_equal(keep[23], got)
    for iters in (1, 5, 23):
        exp, it_o, rn_o = oracle.pcg(rp, col, val, b, x0, precond, 0.0, iters, block_size=bs)
        assert it_o == iters
        assert np.abs(keep[iters] - exp).max() <= 1e-11 * np.abs(exp).max()
        assert abs(hist[iters] - rn_o) <= 1e-11 * rn_o
    # the stopping rule: the same iteration count, the same iterate
    exp, it_o, rn_o = oracle.pcg(rp, col, val, b, None, precond, 1e-9, 4000, block_size=bs)
    got, hist = hp.pcg(rp, col, val, b, None, M, 4000, rtol=1e-9, dtype=np.float64)
    assert len(hist) - 1 == it_o and hist[-1] <= 1e-9 * hist[0] < hist[-2]
    assert np.abs(got - exp).max() <= 1e-9 * np.abs(exp).max()
    # max_iters = 0 and a start vector that solves the system exactly (small integers: b = A x0 without rounding)
    got, hist = hp.pcg(rp, col, val, b, x0, M, 0, dtype=np.float64)
    assert len(hist) == 1 and np.array_equal(got, x0)
    xi = rng.integers(-8, 9, n).astype(np.float64)
    got, hist = hp.pcg(rp, col, val, hp.spmv(rp, col, val, xi, np.float64), xi, M, 20, dtype=np.float64)
    assert len(hist) == 1 and hist[0] == 0.0 and np.array_equal(got, xi)


def test_pcg_isai_application_matches_the_oracle(schwz, oracle):
    """precond 4 of make_precond: W_U (W_L v) with the library's host ISAI values, against the oracle's values on
    the oracle's ILU(0) factors."""
    rp, col, val = oracle.laplacian2d(12)
    n = len(rp) - 1
    v = np.random.default_rng(5).standard_normal(n)
    f = oracle.ilu0(rp, col, val)
    wl, wu = oracle.isai(f["l_rp"], f["l_col"], f["l_val"], True), oracle.isai(f["u_rp"], f["u_col"], f["u_val"], False)
    exp = _csr(dict(u_val=wu, u_col=f["u_col"], u_rp=f["u_rp"]), "u", n) @ (
        _csr(dict(l_val=wl, l_col=f["l_col"], l_rp=f["l_rp"]), "l", n) @ v)
    got = hp.make_precond(schwz, oracle, rp, col, val, 4, 1, np.float64)(v)
    assert np.abs(got - exp).max() <= 1e-13 * np.abs(exp).max()


def test_pcg_longdouble_reaches_the_dense_solution(oracle):
    rng = np.random.default_rng(2)
    rp, col, val = oracle.laplacian2d(6)
    n = len(rp) - 1
    a = sp.csr_matrix((val, col, rp), shape=(n, n)).toarray()
    b = rng.standard_normal(n)
    exp = np.linalg.solve(a, b)
    for M in (hp.precond_none(), hp.precond_jacobi(rp, col, val),
              hp.precond_block_jacobi(rp, col, val, np.arange(0, n + 1, 6))):
        x, hist = hp.pcg(rp, col, val, b, None, M, 10 * n, rtol=1e-17)
        assert x.dtype == np.dtype(LD) and len(hist) - 1 <= n
        assert hist[-1] <= 1e-17 * hist[0]
        assert np.abs(x.astype(np.float64) - exp).max() <= 1e-14 * np.abs(exp).max()
        # the recurred residual norm is the true one while rounding is far away
        x5, h5 = hp.pcg(rp, col, val, b, None, M, 5)
        true = b.astype(LD) - hp.spmv(rp, col, val, x5)
        assert abs(float(h5[-1]) - float(np.sqrt(hp.dot(true, true)))) <= 1e-17 * float(h5[0])


@pytest.mark.parametrize("shape", [(7, 5, 4), (2, 1, 3), (9, 9), (6, 11)])
def test_slicing_stencil_is_the_csr_laplacian_bit_for_bit(oracle, shape):
    if len(shape) == 3:
        rp, col, val = oracle.laplacian3d(*shape)
    elif shape[0] == shape[1]:
        rp, col, val = oracle.laplacian2d(shape[0])
    else:   # a 2-D grid that is not square: the 3-D generator with one plane, its diagonal set to 4
        rp, col, val = oracle.laplacian3d(shape[0], shape[1], 1)
        val = np.where(val > 0, 4.0, val)
    n = len(rp) - 1
    assert n == int(np.prod(shape))
    x = np.random.default_rng(n).standard_normal(n)
    for dtype in (np.float64, LD):
        got = hp.stencil_apply(x.astype(dtype), shape, dtype)
        assert got.dtype == np.dtype(dtype)
        assert np.array_equal(got, hp.spmv(rp, col, val, x, dtype))
    # pcg takes the operator in place of the CSR triple: the same bits
    M = hp.precond_jacobi(rp, col, val, np.float64)
    x_a, h_a = hp.pcg(rp, col, val, x, None, M, 7, dtype=np.float64)
    x_b, h_b = hp.pcg(lambda v: hp.stencil_apply(v, shape, np.float64), None, None, x, None, M, 7, dtype=np.float64)
    assert np.array_equal(x_a, x_b) and h_a == h_b


@pytest.mark.parametrize("me", [0, 1, 2])
def test_slab_operator_is_the_local_matrix(schwz, me):
    """hp.slab_operator with the subdomain's own index set against spmv on its local_matrix: first, middle and last
    slab of 16 x 6 x 18 in three, overlap planes appended behind the interior.  On small integers, where no sum
    rounds, the two are the same bits: the index sets are right.  On random data they are two summation orders of
    the same seven terms (an appended plane has high column numbers, so the CSR row takes it last): within
    7 eps |A| |x| row by row."""
    nx, ny, nz = 16, 6, 18
    prob = schwz.Problem.laplacian(3, nx, ny, nz)
    sd = schwz.Subdomain(prob, 3, me, 2, schwz.partition_regular(prob.N, 3))
    rp, col, val = sd.local_matrix()
    n = len(rp) - 1
    assert n == sd.local_size_x > sd.local_size
    rng = np.random.default_rng(me)
    xi, x = rng.integers(-99, 100, n).astype(np.float64), rng.standard_normal(n)
    for dtype in (np.float64, LD):
        op = hp.slab_operator(sd.local_to_global[:n], nx, ny, dtype)
        assert np.array_equal(op(xi.astype(dtype)), hp.spmv(rp, col, val, xi, dtype))
        mag = hp.spmv(rp, col, np.abs(val), np.abs(x), LD)
        diff = np.abs(op(x.astype(dtype)).astype(LD) - hp.spmv(rp, col, val, x, dtype))
        assert (diff <= 7 * np.finfo(dtype).eps * mag).all()


def test_longdouble_dot_of_2_to_24_terms_against_fsum():
    """The operands are float32 values, so every product is exact in float64 and math.fsum returns the correctly
    rounded sum; fsum of the products and minus that sum gives the rest, hence the exact sum to ~ 2^-106.  The
    pairwise longdouble sum must be within a few longdouble eps of sum |x_i y_i| of it (bound of pairwise summation:
    (log2 n + block) eps; measured here 0.002 eps), where a float64 accumulation is three orders of magnitude off."""
    hp.require_extended_precision()
    n = 1 << 24
    rng = np.random.default_rng(24)
    x = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    y = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    prod = x * y
    assert np.array_equal(prod.astype(LD), x.astype(LD) * y.astype(LD))   # exact products
    s = math.fsum(prod)
    rest = math.fsum(np.append(prod, -s))
    exact = LD(s) + LD(rest)
    mag = LD(np.abs(prod).sum())
    eps = np.finfo(LD).eps
    err = abs(hp.dot(x.astype(LD), y.astype(LD)) - exact)
    print("longdouble pairwise dot: %.3f eps sum|xy|; float64 pairwise: %.1f eps" %
          (float(err / (eps * mag)), float(abs(LD(hp.dot(x, y)) - exact) / (eps * mag))))
    assert err <= 4 * eps * mag


# ---- the row-wise bounds of CSR row sums: they hold for a float64 restatement, and they reject seeded defects ---------

@pytest.fixture(scope="module")
def rowsum_cases():
    hp.require_extended_precision()
    return {name: hp.rowsum_case(name) for name in hp.ROWSUM_CASES}


def _norm_case(kind):
    """An order-1 matrix with x~, b of the RAS norm tests: (rp, col, val, x, b)."""
    rng = np.random.default_rng(77)
    if kind == "band":
        rp, col, val = hp.sym_band_matrix(1500, 6, 40, rng)
    elif kind == "band7":
        rp, col, val = hp.sym_band_matrix(1500, 3, 3, rng)
    else:
        rp, col, val = hp.sym_band_matrix(1501, 14, 60, rng, spd=False)
    n = len(rp) - 1
    return rp, col, val, rng.standard_normal(n), rng.standard_normal(n)


def _sum_sq64(r, L):
    """sum_{i<L} r_i^2 in float64, one term after the other."""
    s = 0.0
    for v in np.asarray(r[:L], dtype=np.float64):
        s += v * v
    return s


def test_the_built_matrices_reach_the_branches_they_are_built_for(rowsum_cases):
    for name, c in rowsum_cases.items():
        assert c["branches"] <= set(hp.tile_branches(c["rp"])), name
    c = rowsum_cases["window2049"]
    t, br = hp.tiles_of(c["rp"]), hp.tile_branches(c["rp"])
    assert br[1] == "b" and t[1] == 1 and t[2] == 3 and c["rp"][1] & 3 == 3 and c["rp"][3] - c["rp"][1] == 2046
    c = rowsum_cases["longrows"]
    t, br, ln = hp.tiles_of(c["rp"]), hp.tile_branches(c["rp"]), np.diff(c["rp"])
    single = {(int(ln[r0]), b) for r0, r1, b in zip(t[:-1], t[1:], br) if r1 - r0 == 1 and ln[r0] > 2000}
    assert single == {(5000, "c"), (2046, "a"), (2047, "a"), (2048, "a"), (2049, "c"), (2047, "c"), (2500, "c")}
    assert ln[0] == 5000 and ln[-1] == 2500
    for name, cap in (("scaled8", 8), ("scaled16", 16), ("scaled32", 32)):
        c = rowsum_cases[name]
        n = len(c["rp"]) - 1
        assert hp.stream_cap(c["rp"]) == cap and n % 4 != 0 and (np.diff(c["rp"]) == 0).any()
        assert np.diff(hp.tiles_of(c["rp"]))[-1] < np.diff(hp.tiles_of(c["rp"]))[0]          # a partial last tile
    assert np.diff(hp.tiles_of(rowsum_cases["scaled32"]["rp"])).max() < 256                    # nnz-limited tiles


def test_row_wise_bounds_hold_for_a_float64_restatement(rowsum_cases):
    """Products rounded, added in CSR order, the epilogue in float64: inside axpby_bound, residual_bound and
    norm_sq_bound on every matrix of the stand-alone SpMV tests."""
    for name, c in rowsum_cases.items():
        a = (c["rp"], c["col"], c["val"], c["x"])
        n = len(c["rp"]) - 1
        for alpha, beta in hp.ALPHA_BETA:
            ref = hp.axpby(*a, alpha, beta, c["y0"])
            got = hp.axpby(*a, alpha, beta, c["y0"], np.float64)
            assert (np.abs(got - ref) <= hp.axpby_bound(*a, alpha, beta, c["y0"])).all(), (name, alpha, beta)
        r, e = hp.residual(*a, c["y0"]), hp.residual_bound(*a, c["y0"])
        r64 = hp.residual(*a, c["y0"], np.float64)
        assert (np.abs(r64 - r) <= e).all(), name
        for L in {n, max(n - 1, 1), (n + 1) // 2}:
            rho2 = np.sum(r[:L] * r[:L])
            assert abs(_sum_sq64(r64, L) - rho2) <= hp.norm_sq_bound(r, e, L), (name, L)
            assert abs(hp.LD(np.sqrt(_sum_sq64(r64, L))) ** 2 - rho2) <= hp.norm_sq_bound(r, e, L, root=True), (name, L)
    for kind in ("band", "band7", "ragged"):
        rp, col, val, x, b = _norm_case(kind)
        r, e, r64 = hp.residual(rp, col, val, x, b), hp.residual_bound(rp, col, val, x, b), hp.residual(rp, col, val, x, b, np.float64)
        for L in (1, 255, 256, 257, len(b) - 1, len(b)):
            assert abs(_sum_sq64(r64, L) - np.sum(r[:L] * r[:L])) <= hp.norm_sq_bound(r, e, L), (kind, L)


def _drop_smallest(rp, col, val, x, bound, small=False):
    """Zero the smallest-magnitude term of one row: the row where that term stands highest above the row's bound, or
    (small) the row with the smallest such term among those where it stands more than four times above it.  Returns
    (val', row, term / bound)."""
    term = np.abs(val * x[col]).astype(hp.LD)
    rows = np.nonzero(np.diff(rp) >= 2)[0]
    at = np.array([rp[i] + int(np.argmin(term[rp[i]:rp[i + 1]])) for i in rows])
    q = term[at] / np.maximum(bound[rows], hp.LD(1e-4000))
    if small:
        ok = np.nonzero(q > 4.0)[0]
        k = ok[int(np.argmin(term[at[ok]]))]
    else:
        k = int(np.argmax(q))
    v = val.copy()
    v[at[k]] = 0.0
    return v, rows[k], float(q[k])


def _round_one_to_fp32(rp, col, val, x, bound):
    rowid = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    change = np.abs((val - val.astype(np.float32).astype(np.float64)) * x[col]).astype(hp.LD)
    q = change / np.maximum(bound[rowid], hp.LD(1e-4000))
    j = int(np.argmax(q))
    v = val.copy()
    v[j] = np.float32(val[j])
    return v, rowid[j], float(q[j])


@pytest.mark.parametrize("name", ["scaled8", "scaled16", "scaled32", "longrows", "window2049"])
def test_row_wise_bounds_reject_a_dropped_term_and_an_fp32_value(rowsum_cases, name):
    """The smallest-magnitude term of one badly scaled row dropped; one matrix value rounded to fp32.  Each defect is
    seeded where it stands more than twice the row's bound high (asserted: the input is chosen, not the bound), and
    on the scaled matrices where 5e-12 max |y|, the tolerance these bounds replace, does not see the dropped term."""
    c = rowsum_cases[name]
    rp, col, val, x, y0 = c["rp"], c["col"], c["val"], c["x"], c["y0"]
    for alpha, beta in ((1.0, 0.0), (0.5, -2.0)):
        ref = hp.axpby(rp, col, val, x, alpha, beta, y0)
        bound = hp.axpby_bound(rp, col, val, x, alpha, beta, y0)
        for seed in (_drop_smallest, _round_one_to_fp32):
            v, row, q = seed(rp, col, val, x, bound / abs(alpha))
            assert q > 2.0, (seed.__name__, q)
            got = hp.axpby(rp, col, v, x, alpha, beta, y0, np.float64)
            assert abs(got[row] - ref[row]) > bound[row], seed.__name__
        if name.startswith("scaled"):
            v, row, q = _drop_smallest(rp, col, val, x, bound / abs(alpha), small=True)
            got = hp.axpby(rp, col, v, x, alpha, beta, y0, np.float64)
            assert q > 4.0 and abs(got[row] - ref[row]) > bound[row]
            assert abs(got[row] - ref[row]) < 1e-30 * 5e-12 * float(np.abs(ref).max())    # ... and far below
    r, e = hp.residual(rp, col, val, x, y0), hp.residual_bound(rp, col, val, x, y0)
    for seed in (_drop_smallest, _round_one_to_fp32):
        v, row, q = seed(rp, col, val, x, e)
        assert q > 2.0
        assert abs(hp.residual(rp, col, v, x, y0, np.float64)[row] - r[row]) > e[row]


@pytest.mark.parametrize("kind", ["band", "band7", "ragged"])
def test_norm_bound_rejects_the_seeded_defects(kind):
    """On the order-1 matrices of the norm tests: a dropped term, an fp32 value, and a row limit off by one in either
    direction at 1, 255, 256, 257, n - 1 change the sum of squares by more than norm_sq_bound allows."""
    hp.require_extended_precision()
    rp, col, val, x, b = _norm_case(kind)
    n = len(b)
    r, e = hp.residual(rp, col, val, x, b), hp.residual_bound(rp, col, val, x, b)
    r64 = hp.residual(rp, col, val, x, b, np.float64)
    for L in (1, 255, 256, 257, n - 1):
        B = hp.norm_sq_bound(r, e, L, root=True)
        rho2 = np.sum(r[:L] * r[:L])
        assert r[L - 1] ** 2 > 4 * B and r[L] ** 2 > 4 * B           # the discrimination condition
        assert abs(_sum_sq64(r64, L) - rho2) <= B
        assert abs(_sum_sq64(r64, L + 1) - rho2) > B                   # row <= row_limit
        assert L == 1 or abs(_sum_sq64(r64, L - 1) - rho2) > B         # row < row_limit - 1
    B, rho2 = hp.norm_sq_bound(r, e, n), np.sum(r * r)
    # a defect in row i moves the sum by about 2 |r_i| d: seed it where that is largest against B
    weight = 2 * np.abs(r) / B
    for seed in (_drop_smallest, _round_one_to_fp32):
        v, row, q = seed(rp, col, val, x, 1 / np.maximum(weight, hp.LD(1e-300)))
        assert q > 4.0, (seed.__name__, q)
        assert abs(_sum_sq64(hp.residual(rp, col, v, x, b, np.float64), n) - rho2) > B, seed.__name__


def test_residual_bound_rejects_a_skipped_first_entry_of_an_interface_row():
    """The interface update b~_i = b_i - (A_Gamma x~)_i on a badly scaled rectangular matrix (the rows 500..999 of a
    scaled band matrix, the columns outside them): the loop started at rp[i] + 1 in one row."""
    hp.require_extended_precision()
    rng = np.random.default_rng(12)
    rp, col, val = hp.sym_band_matrix(1500, 6, 40, rng, spd=False)
    val, s, _ = hp.rescale_rows_cols(rp, col, val, rng)
    a = sp.csr_matrix((val, col, rp), shape=(1500, 1500))[500:1000].tocsc()
    a = sp.hstack([a[:, :500], a[:, 1000:]]).tocsr()
    a.sort_indices()
    irp, icol, ival = a.indptr, a.indices, a.data
    assert a.nnz > 100 and (np.diff(irp) == 0).any()
    x = rng.standard_normal(1000)
    b = np.ldexp(rng.standard_normal(500), s[500:1000])
    r, e = hp.residual(irp, icol, ival, x, b), hp.residual_bound(irp, icol, ival, x, b)
    assert (np.abs(hp.residual(irp, icol, ival, x, b, np.float64) - r) <= e).all()
    first = irp[:-1][np.diff(irp) > 0]
    rows = np.nonzero(np.diff(irp) > 0)[0]
    q = np.abs(ival[first] * x[icol[first]]) / e[rows]
    # (a first entry 2^-60 of its row is rounding noise to any bound; most are not)
    seen = np.nonzero(q > 2.0)[0]
    assert len(seen) > len(rows) // 2
    for k in (seen[0], seen[len(seen) // 2], seen[-1]):
        v = ival.copy()
        v[first[k]] = 0.0
        got = hp.residual(irp, icol, v, x, b, np.float64)
        assert abs(got[rows[k]] - r[rows[k]]) > e[rows[k]]


# ---- the coarse correction: residual of the aggregates, dense GEMV, apply ------------------------------------------------

PIECE_TARGETS = (2047, 2048, 2049, 4096, 4097)


@pytest.fixture(scope="module")
def coarse_case():
    """hp.sym_band_matrix(16384, 6, 40, default_rng(7)), x~ = +-u, contiguous aggregates of one row, then exactly
    2047, 2048, 2049, 4096, 4097 W entries, then the rest: aggregates of 1, 2 and 3 pieces."""
    hp.require_extended_precision()
    rng = np.random.default_rng(7)
    rp, col, val = hp.sym_band_matrix(16384, 6, 40, rng)
    n = len(rp) - 1
    x = hp.pow2_operands(rng, n)
    b = hp.pow2_operands(rng, n)
    agg = hp.aggregates_by_w_count(rp, col, (int(rp[1]),) + PIECE_TARGETS)
    m = int(agg.max()) + 1
    w_ptr, w_slot, w_val, beta = hp.coarse_w(rp, col, val, b, agg, m)
    assert tuple(np.diff(w_ptr)[:6]) == (int(rp[1]),) + PIECE_TARGETS and m == 7
    pieces, piece_ptr = hp.coarse_pieces(w_ptr)
    assert set(np.diff(piece_ptr)) == {1, 2, 3}
    return dict(rp=rp, col=col, val=val, x=x, b=b, agg=agg, m=m, w=(w_ptr, w_slot, w_val, beta), pieces=pieces,
                piece_ptr=piece_ptr, s=hp.coarse_residual(rp, col, val, x, b, agg, m),
                e=hp.coarse_residual_bound(rp, col, val, x, b, agg, m))


def test_coarse_residual_bound_holds_for_float64_restatements_in_any_order(coarse_case):
    """The plan's order -- W summed first, pieces of at most 2048 entries, a tree inside a piece, the fold in table
    order -- and three random orders of the W entries, summed one after the other."""
    c = coarse_case
    w_ptr, w_slot, w_val, beta = c["w"]
    got = hp.coarse_residual64(w_ptr, w_slot, w_val, beta, c["x"])
    q = np.abs(got - c["s"]) / c["e"]
    print("\ncoarse residual, plan order: error / bound per aggregate", np.asarray(q, dtype=np.float64))
    assert (q <= 1.0).all()
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        s = np.zeros(c["m"])
        for a in range(c["m"]):
            k = w_ptr[a] + rng.permutation(w_ptr[a + 1] - w_ptr[a])
            t = 0.0
            for v in w_val[k] * c["x"][w_slot[k]]:
                t += v
            s[a] = beta[a] - t
        assert (np.abs(s - c["s"]) <= c["e"]).all(), seed
    # the definition itself in float64: rows in CSR order, no W at all
    s64 = hp.coarse_residual(c["rp"], c["col"], c["val"], c["x"], c["b"], c["agg"], c["m"], np.float64)
    assert (np.abs(s64 - c["s"]) <= c["e"]).all()


def test_coarse_residual_bound_rejects_the_seeded_piece_defects(coarse_case):
    """The last entry of a piece dropped; one piece left out of the fold; the fold adding the first piece of the next
    aggregate.  What each defect removes or adds is asserted to be more than 4 e_a first: on the input."""
    c = coarse_case
    w_ptr, w_slot, w_val, beta = c["w"]
    pieces, piece_ptr, e = c["pieces"], c["piece_ptr"], c["e"]
    term = np.abs(w_val * c["x"][w_slot]).astype(LD)
    for a in range(1, c["m"]):
        assert term[w_ptr[a]:w_ptr[a + 1]].min() > 4 * e[a], a          # no entry of these aggregates is negligible
    partial = np.array([hp.block_tree_sum64((w_val * c["x"][w_slot])[b0:b1]) for _, b0, b1 in pieces])
    for p, (a, b0, b1) in enumerate(pieces):
        if a == 0:
            continue
        # the last entry of piece p dropped
        short = list(pieces)
        short[p] = (a, b0, b1 - 1)
        got = hp.coarse_residual64(w_ptr, w_slot, w_val, beta, c["x"], short, piece_ptr)
        assert abs(got[a] - c["s"][a]) > e[a], ("dropped entry", p)
        assert (np.abs(np.delete(got, a) - np.delete(c["s"], a)) <= np.delete(e, a)).all()
    for a in range(1, c["m"]):
        # the fold stops one piece early
        assert abs(partial[piece_ptr[a + 1] - 1]) > 4 * e[a], a
        early = piece_ptr.copy()
        table = [q for k, q in enumerate(pieces) if k != piece_ptr[a + 1] - 1]
        early[a + 1:] -= 1
        got = hp.coarse_residual64(w_ptr, w_slot, w_val, beta, c["x"], table, early)
        assert abs(got[a] - c["s"][a]) > e[a], ("piece left out", a)
        # the fold runs one piece too far: the next aggregate's first piece
        if a + 1 < c["m"]:
            assert abs(partial[piece_ptr[a + 1]]) > 4 * e[a], a
            got = _fold_one_too_far(c, a)
            assert abs(got - c["s"][a]) > e[a], ("neighbour's piece", a)


def _fold_one_too_far(c, a):
    w_ptr, w_slot, w_val, beta = c["w"]
    t = w_val * c["x"][w_slot]
    f = 0.0
    for p in range(int(c["piece_ptr"][a]), int(c["piece_ptr"][a + 1]) + 1):
        f += hp.block_tree_sum64(t[c["pieces"][p][1]:c["pieces"][p][2]])
    return beta[a] - f


def _gemv_operands(nc, seed):
    """M_ij = +-u 2^(e_i + f_j), s_j = +-u 2^-f_j, e and f in [-20, 20]: badly scaled operands, comparable terms."""
    rng = np.random.default_rng(seed)
    e, f = rng.integers(-20, 21, nc), rng.integers(-20, 21, nc)
    M = hp.pow2_operands(rng, nc * nc, exps=(e[:, None] + f[None, :]).reshape(-1)).reshape(nc, nc)
    return M, hp.pow2_operands(rng, nc, exps=-f)


def _gemv_lanes64(M, s, skip=()):
    """One wave per row: lane l adds its columns l, l + 64, ..., the lanes fold by halves."""
    nc = M.shape[0]
    lanes = np.zeros((nc, 64))
    for k0 in range(0, nc, 64):
        p = M[:, k0:k0 + 64] * s[k0:k0 + 64]
        for j in skip:
            if k0 <= j < k0 + 64:
                p[:, j - k0] = 0.0
        lanes[:, :p.shape[1]] += p
    off = 32
    while off:
        lanes[:, :off] += lanes[:, off:2 * off]
        off >>= 1
    return lanes[:, 0].copy()


def _pairwise64(p):
    while p.shape[1] > 1:
        if p.shape[1] & 1:
            p = np.concatenate([p, np.zeros((p.shape[0], 1))], axis=1)
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


@pytest.mark.parametrize("nc", [1, 3, 65, 129, 130, 513])
def test_coarse_gemv_bound_holds_and_rejects_a_skipped_column(nc):
    hp.require_extended_precision()
    M, s = _gemv_operands(nc, 100 + nc)
    ref, mag = hp.coarse_gemv(M, s, block=100)
    bound = hp.coarse_gemv_bound(mag, nc)
    for got in (_gemv_lanes64(M, s), _pairwise64(M * s), M @ s):
        assert (np.abs(got - ref) <= bound).all(), nc
    skips = ([64] if nc > 64 else []) + ([nc - 1] if nc & 1 and nc > 1 else [])
    for j in skips:
        assert (np.abs(M[:, j] * s[j]) > 4 * bound).all(), (nc, j)          # on the input: every row shows it
        assert (np.abs(_gemv_lanes64(M, s, skip=(j,)) - ref) > bound).all(), (nc, j)


def test_coarse_apply_reference_is_exact_and_the_seeded_defects_differ_in_bits():
    """x~ + c[agg] is one rounded addition: the reference is the same float64 expression.  Slot nx - 1 skipped, c
    added twice, ids read shifted by one: each differs in bits, asserted on the operands first."""
    rng = np.random.default_rng(5)
    nx, ny, nc = 1001, 777, 37
    x, y, c = (hp.pow2_operands(rng, k, -20, 20) for k in (nx, ny, nc))
    ids = rng.integers(0, nc, nx)
    want_x, want_y = hp.coarse_apply(x, y, c, ids)
    exact = x.astype(LD) + c[ids].astype(LD)
    assert np.array_equal(want_x, exact.astype(np.float64))                  # one rounding of the exact sum
    # operands spread over 2^42 at most: no c is absorbed by its x~, once or twice
    assert (want_x != x).all() and (want_y != y).all() and (want_x + c[ids] != want_x).all()
    skipped = want_x.copy()
    skipped[nx - 1] = x[nx - 1]
    assert not np.array_equal(skipped.view(np.int64), want_x.view(np.int64))
    twice = want_y + c[ids[:ny]]
    assert (twice.view(np.int64) != want_y.view(np.int64)).all()
    shifted = x[:-1] + c[ids[1:]]
    differ = ids[1:] != ids[:-1]
    assert differ.any() and (c[ids[1:]][differ] != c[ids[:-1]][differ]).all()
    assert (shifted[differ].view(np.int64) != want_x[:-1][differ].view(np.int64)).any()
