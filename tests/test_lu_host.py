"""CPU tests of the host sparse LU with threshold partial pivoting (schwz_lu, the factorization
behind --local_factorization=umfpack) and of the solver-name mapping that selects it."""
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(__file__), "golden")


def _csr(rp, col, val):
    import scipy.sparse as sp
    n = len(rp) - 1
    return sp.csr_matrix((np.asarray(val, dtype=np.float64), np.asarray(col), np.asarray(rp)), shape=(n, n))


def _golden(name):
    if name == "lap2d_16":  # lap2d_16.npz holds the solution; the matrix is the generated Laplacian
        import oracle as O
        return O.laplacian2d(16)
    g = np.load(os.path.join(G, name + ".npz"))
    return g["rp"], g["col"], g["val"]


def _shifted_convdiff(convdiff, n):
    """convdiff rows shifted cyclically by two (no stencil offset): every diagonal entry is zero, so the factorization
    has to pivot."""
    import scipy.sparse as sp
    a = _csr(*convdiff(n)).tolil()
    N = a.shape[0]
    b = sp.csr_matrix(a[np.roll(np.arange(N), 2), :])
    b.sort_indices()
    assert np.all(b.diagonal() == 0.0)
    return b.indptr.astype(np.int32), b.indices.astype(np.int32), b.data.astype(np.float64)


def _check_factors(A, f):
    n = A.shape[0]
    p, q = f["row_perm"], f["col_perm"]
    for perm in (p, q):
        assert np.array_equal(np.sort(perm), np.arange(n))
    for i in range(n):
        lc = f["l_col"][f["l_rp"][i]:f["l_rp"][i + 1]]
        lv = f["l_val"][f["l_rp"][i]:f["l_rp"][i + 1]]
        uc = f["u_col"][f["u_rp"][i]:f["u_rp"][i + 1]]
        assert len(lc) and lc[-1] == i and lv[-1] == 1.0 and np.all(lc[:-1] < i)
        assert len(uc) and uc[0] == i and np.all(uc[1:] > i)
        assert np.all(np.diff(lc) > 0) and np.all(np.diff(uc) > 0)
    L = _csr(f["l_rp"], f["l_col"], f["l_val"])
    U = _csr(f["u_rp"], f["u_col"], f["u_val"])
    R = A[p, :][:, q] - L @ U
    norm = abs(A).sum(axis=1).max()
    assert abs(R).sum(axis=1).max() <= 1e-13 * norm


def _cases(convdiff):
    return {"convdiff20": convdiff(20), "lap2d_16": _golden("lap2d_16"), "ani3_crop": _golden("ani3_crop"),
            "shifted": _shifted_convdiff(convdiff, 20)}


@pytest.mark.parametrize("case", ["convdiff20", "lap2d_16", "ani3_crop", "shifted"])
@pytest.mark.parametrize("natural", [False, True])
def test_lu_factors_the_matrix(schwz, convdiff, case, natural):
    rp, col, val = _cases(convdiff)[case]
    A = _csr(rp, col, val)
    f = schwz.lu(rp, col, val, natural=natural)
    _check_factors(A, f)
    if case == "shifted":
        assert not np.array_equal(f["row_perm"], f["col_perm"])
    if natural:
        assert np.array_equal(f["col_perm"], np.arange(A.shape[0]))


@pytest.mark.parametrize("case", ["convdiff20", "lap2d_16", "ani3_crop", "shifted"])
def test_lu_solve_matches_spsolve(schwz, convdiff, case):
    import scipy.sparse.linalg as sl
    rp, col, val = _cases(convdiff)[case]
    A = _csr(rp, col, val)
    n = A.shape[0]
    f = schwz.lu(rp, col, val)
    L = _csr(f["l_rp"], f["l_col"], f["l_val"])
    U = _csr(f["u_rp"], f["u_col"], f["u_val"])
    b = np.random.default_rng(3).standard_normal(n)
    w = sl.spsolve_triangular(L, b[f["row_perm"]], lower=True)
    z = sl.spsolve_triangular(U, w, lower=False)
    y = np.empty(n)
    y[f["col_perm"]] = z
    x = sl.spsolve(A.tocsc(), b)
    assert np.abs(y - x).max() <= 1e-11 * np.abs(x).max()


def test_natural_ordering_keeps_a_dominant_diagonal(schwz, convdiff):
    """convdiff's diagonal always passes the 0.1 threshold: no row moves either."""
    rp, col, val = convdiff(20)
    f = schwz.lu(rp, col, val, natural=True)
    n = len(rp) - 1
    assert np.array_equal(f["col_perm"], np.arange(n))
    assert np.array_equal(f["row_perm"], np.arange(n))


def test_symmetric_pattern_uses_the_ll_t_ordering(schwz):
    """On a symmetric matrix the column pre-order is the LL^T one (RCM of A's pattern)."""
    rp, col, val = _golden("lap2d_16")
    f = schwz.lu(rp, col, val)
    c = schwz.cholesky(rp, col, val)
    assert np.array_equal(f["col_perm"], c["perm"])
    assert np.array_equal(f["row_perm"], c["perm"])


def test_singular_matrices_are_refused(schwz, convdiff):
    import scipy.sparse as sp
    rp, col, val = convdiff(8)
    A = _csr(rp, col, val).tolil()
    empty = A.copy()
    empty[:, 5] = 0.0
    twins = A.copy()
    twins[6, :] = A[5, :]
    for M in (empty, twins):
        M = sp.csr_matrix(M)
        M.eliminate_zeros()
        M.sort_indices()
        for natural in (False, True):
            with pytest.raises(schwz.SchwzError) as e:
                schwz.lu(M.indptr, M.indices, M.data, natural=natural)
            assert e.value.code == schwz.capi.ERR_NOT_SPD


def test_umfpack_factorization_selects_the_lu(schwz):
    from schwz_amd import solver as sv
    code = lambda **kw: sv._factor_solver_code(schwz.Settings(**kw))
    assert code(local_solver="direct-ginkgo", factorization="umfpack") == schwz.capi.SOLVER_DIRECT_LU
    assert code(local_solver="direct-cholmod", factorization="umfpack") == schwz.capi.SOLVER_DIRECT_LU
    assert code(local_solver="direct-ginkgo", factorization="umfpack",
                non_symmetric_matrix=True) == schwz.capi.SOLVER_DIRECT_LU
    assert code(local_solver="direct-ginkgo") == schwz.capi.SOLVER_DIRECT
    assert code(local_solver="iterative-ginkgo", factorization="umfpack") == schwz.capi.SOLVER_ITERATIVE
    with pytest.raises(schwz.capi.NotImplementedSchwz):
        code(local_solver="direct-ginkgo", non_symmetric_matrix=True)
    with pytest.raises(schwz.capi.NotImplementedSchwz):
        code(local_solver="direct-umfpack", factorization="umfpack")


def test_trs_create_lu_validates_on_the_host(schwz):
    """Both permutations are required and range-checked before any device call."""
    import ctypes as C
    f = schwz.lu(*_golden("lap2d_16"))
    bad = f["col_perm"].copy()
    bad[0] = len(bad)
    for rperm, cperm in ((f["row_perm"], bad), (bad, f["col_perm"])):
        with pytest.raises(schwz.SchwzError) as e:
            schwz.TrsLU(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"], rperm, cperm)
        assert e.value.code == schwz.capi.ERR_INVALID
    h = C.c_void_p()
    args = [np.ascontiguousarray(f[k]) for k in ("l_rp", "l_col", "l_val", "u_rp", "u_col", "u_val", "row_perm")]
    rc = schwz.capi.lib.schwz_trs_create_lu(len(f["l_rp"]) - 1, *[schwz.capi.ptr(a) for a in args], None,
                                            C.byref(h))
    assert rc == schwz.capi.ERR_INVALID
