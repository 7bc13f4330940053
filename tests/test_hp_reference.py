"""The extended-precision references of hp_reference.py, pinned on the CPU: against scipy, against the C
oracle, against a dense solve, and the componentwise substitution bound against a float64 run of the same
substitution (it must hold, and it must not be slack by orders of magnitude)."""
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
