"""BiCGSTAB as the local solver of non-symmetric matrices (Metadata.non_symmetric_solver, schwz_bicgstab_create,
schwz_ras_set_nonsym_solver): the default, what the host accepts and refuses before any device call, the argument
checks of the C ABI that need no GPU, and the reference restatement of tests/hp_bicgstab.py pinned by scipy and by
four cases that can be checked by hand."""
import ctypes

import numpy as np
import pytest

import hp_bicgstab
import hp_reference as hp
from conftest import convection_diffusion_2d


def test_metadata_field_defaults_to_gmres(schwz):
    assert schwz.Metadata().non_symmetric_solver == "gmres"


def _code(schwz, settings_kw=None, **metadata_kw):
    from schwz_amd import solver as sv
    return sv._nonsym_solver_code(schwz.Settings(**(settings_kw or {})), schwz.Metadata(**metadata_kw))


def test_accepted_combinations(schwz):
    c = schwz.capi
    assert (c.NONSYM_GMRES, c.NONSYM_BICGSTAB) == (0, 1)
    nonsym = dict(non_symmetric_matrix=True)
    assert _code(schwz) == c.NONSYM_GMRES
    assert _code(schwz, nonsym) == c.NONSYM_GMRES
    assert _code(schwz, nonsym, non_symmetric_solver="gmres") == c.NONSYM_GMRES
    assert _code(schwz, nonsym, non_symmetric_solver="bicgstab") == c.NONSYM_BICGSTAB
    for pc in (dict(local_precond="null"), dict(local_precond="block-jacobi", precond_max_block_size=1),
               dict(local_precond="block-jacobi", precond_max_block_size=8), dict(local_precond="ilu"),
               dict(local_precond="isai"), dict(local_precond="ilu", par_ilu_sweeps=3, trisolve_sweeps=2)):
        assert _code(schwz, nonsym, non_symmetric_solver="bicgstab", **pc) == c.NONSYM_BICGSTAB


def test_the_field_has_no_effect_without_the_non_symmetric_iterative_solver(schwz):
    """Like restart_iter: a symmetric matrix keeps its CG, a direct local solver its factors."""
    c = schwz.capi
    assert _code(schwz, non_symmetric_solver="bicgstab") == c.NONSYM_GMRES
    assert _code(schwz, dict(local_solver="direct-ginkgo"), non_symmetric_solver="bicgstab") == c.NONSYM_GMRES
    assert _code(schwz, dict(non_symmetric_matrix=True, local_solver="direct-ginkgo", factorization="umfpack"),
                 non_symmetric_solver="bicgstab") == c.NONSYM_GMRES


@pytest.mark.parametrize("settings_kw", [dict(), dict(non_symmetric_matrix=True), dict(local_solver="direct-ginkgo")])
@pytest.mark.parametrize("name", ["cgs", "BiCGSTAB", "GMRES", "", None, 1])
def test_unknown_solver_name_is_invalid(schwz, name, settings_kw):
    with pytest.raises(schwz.SchwzError) as e:
        _code(schwz, settings_kw, non_symmetric_solver=name)
    assert e.value.code == schwz.capi.ERR_INVALID
    assert not isinstance(e.value, schwz.NotImplementedSchwz)


def test_initialize_refuses_before_any_device_call(schwz):
    """The validator runs at the top of initialize(): no matrix is set up, no subdomain created."""
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(4, 4, 4), non_symmetric_matrix=True)
    m = schwz.Metadata(num_subdomains=1, non_symmetric_solver="bicg")

    class NoBackend:
        def __getattr__(self, name):
            raise AssertionError("the backend was touched: %s" % name)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(1), backend=NoBackend(), quiet=True)
    with pytest.raises(schwz.SchwzError) as e:
        solver.initialize()
    assert e.value.code == schwz.capi.ERR_INVALID


def test_capi_refuses_before_touching_the_matrix(schwz):
    """schwz_bicgstab_create runs the checks of schwz_gmres_create_ex on the preconditioner code, the ParILU options
    and the output pointer before it looks at the matrix."""
    lib, c = schwz.capi.lib, schwz.capi
    h = ctypes.c_void_p()
    create = lib.schwz_bicgstab_create
    for args in ((c.PRECOND_JACOBI, 1, 0, 0), (99, 1, 0, 0), (-1, 1, 0, 0), (c.PRECOND_ILU, 1, -1, 0),
                 (c.PRECOND_ILU, 1, 0, -2), (c.PRECOND_JACOBI, 1, 2, 0), (c.PRECOND_ISAI, 1, 0, 3),
                 (c.PRECOND_ILU, 1, 2, 2)):
        want = lib.schwz_gmres_create_ex(None, args[0], args[1], 4, args[2], args[3], ctypes.byref(h))
        assert want != c.OK
        assert create(None, *args, ctypes.byref(h)) == want, args
        assert not h.value
    assert create(None, c.PRECOND_ILU, 1, -1, 0, ctypes.byref(h)) == c.ERR_INVALID
    assert create(None, c.PRECOND_JACOBI, 1, 2, 0, ctypes.byref(h)) == c.ERR_NOT_IMPLEMENTED
    assert create(None, c.PRECOND_JACOBI, 1, 0, 0, None) == c.ERR_INVALID          # null output pointer
    assert create(None, c.PRECOND_JACOBI, 1, 0, 0, ctypes.byref(h)) == c.ERR_INVALID   # ... and null matrix
    assert lib.schwz_bicgstab_breakdown(None) == 0
    lib.schwz_bicgstab_destroy(None)
    # no subdomain: GMRES, and nothing to set
    assert lib.schwz_ras_nonsym_solver(None) == c.NONSYM_GMRES
    assert lib.schwz_ras_set_nonsym_solver(None, c.NONSYM_BICGSTAB) == c.ERR_INVALID
    assert lib.schwz_ras_set_nonsym_solver(None, 7) == c.ERR_INVALID


def test_setter_needs_a_subdomain_on_the_device(schwz):
    p = schwz.Problem.laplacian(2, 8)
    sd = schwz.Subdomain(p, 1, 0, 2, schwz.partition_regular(64, 1))
    with pytest.raises(schwz.SchwzError) as e:
        sd.set_nonsym_solver(schwz.capi.NONSYM_BICGSTAB)
    assert e.value.code == schwz.capi.ERR_INVALID
    with pytest.raises(schwz.SchwzError) as e:
        sd.set_nonsym_solver(5)
    assert e.value.code == schwz.capi.ERR_INVALID
    assert sd.nonsym_solver() == schwz.capi.NONSYM_GMRES


def test_solver_options_are_unchanged(schwz):
    """The choice travels through schwz_ras_set_nonsym_solver: the options struct keeps its layout."""
    assert [n for n, _ in schwz.capi.SolverOptions._fields_] == [
        "local_solver", "precond", "local_tol", "local_max_iters", "natural_factor_ordering", "spmv_variant",
        "precond_block_size", "non_symmetric", "restart_iter", "par_ilu_sweeps", "trisolve_sweeps"]
    assert ctypes.sizeof(schwz.capi.SolverOptions) == 48


def test_poll_batch_matches_the_header(schwz):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "schwz_hip.h")).read()
    assert int(re.search(r"#define SCHWZ_BICGSTAB_POLL_BATCH (\d+)", header).group(1)) == \
        schwz.capi.BICGSTAB_POLL_BATCH


# ---- the restatement ---------------------------------------------------------------------------------------

def _csr(rp, col, val):
    import scipy.sparse as sp
    n = len(rp) - 1
    return sp.csr_matrix((np.asarray(val, dtype=np.float64), np.asarray(col), np.asarray(rp)), shape=(n, n))


def test_restatement_agrees_with_scipy():
    import scipy.sparse.linalg as sl
    rp, col, val = convection_diffusion_2d(30)
    n = len(rp) - 1
    A = _csr(rp, col, val)
    b = np.random.default_rng(29).standard_normal(n)
    M = hp.make_precond(None, None, rp, col, val, 1, 1, np.float64)
    x, hist, half, bd = hp_bicgstab.bicgstab(rp, col, val, b, None, M, 10 * n, 1e-10, np.float64)
    assert bd == 0 and len(hist) - 1 < 10 * n
    exact = sl.spsolve(A.tocsc(), b)
    assert np.abs(x - exact).max() <= 1e-8 * np.abs(exact).max()
    count = [0]

    def cb(_):
        count[0] += 1
    Mop = sl.LinearOperator((n, n), matvec=lambda w: M(w))
    try:
        xs, info = sl.bicgstab(A, b, rtol=1e-10, atol=0.0, M=Mop, callback=cb, maxiter=10 * n)
    except TypeError:   # older scipy: the relative tolerance is `tol`
        xs, info = sl.bicgstab(A, b, tol=1e-10, atol=0.0, M=Mop, callback=cb, maxiter=10 * n)
    assert info == 0
    print("restatement: %d iterations, scipy: %d callbacks" % (len(hist) - 1, count[0]))
    assert abs((len(hist) - 1) - count[0]) <= 1


@pytest.mark.parametrize("dtype", [np.float64, hp.LD])
def test_restatement_by_hand(dtype):
    none = hp.precond_none(dtype)
    # A = 2 I: v = 2 r, alpha = 1/2, s = 0 exactly: the half step of iteration 0 ends the solve
    rp, col, val = np.arange(4), np.arange(3), np.full(3, 2.0)
    b = np.array([1.0, -3.0, 5.0])
    x, hist, half, bd = hp_bicgstab.bicgstab(rp, col, val, b, None, none, 5, 0.0, dtype)
    assert len(hist) - 1 == 1 and bd == 0 and hist[-1] == 0 and half == [0]
    assert np.array_equal(np.asarray(x, dtype=np.float64), b / 2)
    # the skew matrix: rhat.v = r.(A r) = 0 exactly
    rp, col, val = np.array([0, 1, 2]), np.array([1, 0]), np.array([1.0, -1.0])
    b, x0 = np.array([3.0, 4.0]), np.array([0.5, -0.25])
    x, hist, half, bd = hp_bicgstab.bicgstab(rp, col, val, b, x0, none, 5, 0.0, dtype)
    assert bd == 2 and len(hist) - 1 == 0 and half == []
    assert np.array_equal(np.asarray(x, dtype=np.float64), x0)
    # b = A x0 in small integers: the top test of iteration 0
    rp, col, val = convection_diffusion_2d(6, 2.0, -1.0)
    x0 = np.arange(36, dtype=np.float64) - 17
    b = np.asarray(hp.spmv(rp, col, val, x0, np.float64))
    x, hist, half, bd = hp_bicgstab.bicgstab(rp, col, val, b, x0, none, 5, 0.0, dtype)
    assert bd == 0 and len(hist) - 1 == 0 and hist[0] == 0
    assert np.array_equal(np.asarray(x, dtype=np.float64), x0)
    # max_iters = 0
    b = np.ones(36)
    x, hist, half, bd = hp_bicgstab.bicgstab(rp, col, val, b, x0, none, 0, 1e-8, dtype)
    assert bd == 0 and len(hist) == 1 and hist[0] > 0
    assert np.array_equal(np.asarray(x, dtype=np.float64), x0)
