"""Chebyshev as a local solver of symmetric matrices (Metadata.symmetric_solver, schwz_cheb_create,
schwz_ras_set_sym_solver): the restatement of tests/hp_chebyshev.py pinned by the closed form of the Chebyshev
polynomial, the default, what the host accepts and refuses before any device call, and the argument checks of the C
ABI that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import hp_chebyshev
import hp_reference as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["schwz_cheb_create", "schwz_cheb_destroy", "schwz_cheb_bounds", "schwz_cheb_set_bounds",
               "schwz_cheb_solve", "schwz_cheb_last_stats", "schwz_ras_set_sym_solver", "schwz_ras_sym_solver",
               "schwz_ras_cheb_bounds", "schwz_ras_set_cheb_bounds"]


# ---- the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [hp.LD, np.float64])
@pytest.mark.parametrize("m", [1, 2, 7, 25])
def test_restatement_is_the_chebyshev_polynomial(m, dtype):
    """A = diag(lambda_i), M = I, x_0 = 0, b = 1: x_m,i = (1 - T_m((theta - lambda_i) / delta) / T_m(sigma)) / lambda_i.
    37 eigenvalues in [0.05, 1.9] with the bounds [0.1, 2.0]: some lie below lmin on purpose (they are damped too, only
    more slowly).  Agreement to 1e-12 (a float64 run of the same recurrence gave 3e-15 to 2e-14)."""
    from numpy.polynomial.chebyshev import chebval
    if dtype is hp.LD:
        hp.require_extended_precision()
    lam = np.linspace(0.05, 1.9, 37)
    n = len(lam)
    lmin, lmax = 0.1, 2.0
    rp, col = np.arange(n + 1), np.arange(n)
    x, hist = hp_chebyshev.chebyshev(rp, col, lam, np.ones(n), None, None, lmin, lmax, m, 0.0, dtype)
    assert len(hist) - 1 == m
    L = lam.astype(hp.LD)
    theta, delta = (hp.LD(lmax) + hp.LD(lmin)) / 2, (hp.LD(lmax) - hp.LD(lmin)) / 2
    coef = np.zeros(m + 1, dtype=hp.LD)
    coef[m] = 1
    want = (1 - chebval((theta - L) / delta, coef) / chebval(theta / delta, coef)) / L
    err = float(np.abs(x.astype(hp.LD) - want).max() / np.abs(want).max())
    print("m = %d %s: %.2e" % (m, np.dtype(dtype).name, err))
    assert err <= 1e-12
    # the recurred residual is the true one: r_m,i = T_m(.) / T_m(sigma)
    r = 1 - L * x.astype(hp.LD)
    assert abs(float(np.sqrt(np.dot(r, r))) - float(hist[-1])) <= 1e-12 * float(hist[0])


def test_restatement_converges_on_the_laplacian(oracle):
    """lap3d_12x12x12 with Jacobi and the bounds [2/30, 2] (2 is the Gershgorin bound of D^-1 A; the smallest
    eigenvalue, 1 - cos(pi / 13) = 0.029, lies below lmin): after 200 corrections the TRUE residual is below 1e-8 of the
    start."""
    rp, col, val = oracle.laplacian3d(12, 12, 12)
    n = len(rp) - 1
    diag = hp_chebyshev.diagonal(rp, col, val)
    assert hp_chebyshev.gershgorin(rp, col, val, diag) == 2.0
    b = np.random.default_rng(3).standard_normal(n)
    x, hist = hp_chebyshev.chebyshev(rp, col, val, b, None, diag, 2.0 / 30.0, 2.0, 200, 0.0, np.float64)
    true = b - hp.spmv(rp, col, val, x, np.float64)
    assert len(hist) - 1 == 200
    assert np.linalg.norm(true) <= 1e-8 * float(hist[0])
    assert float(hist[-1]) <= 1e-8 * float(hist[0])


def test_restatement_stop_rule():
    """Checked iterates are k = 0 (mod 8) and k = m: a loose tolerance stops at 8, never at 1 ... 7; a zero start
    residual stops at 0; max_iters = 0 returns x_0."""
    n = 20
    rp, col, val = np.arange(n + 1), np.arange(n), np.linspace(0.5, 1.5, n)
    b = np.ones(n)
    x, hist = hp_chebyshev.chebyshev(rp, col, val, b, None, None, 0.4, 1.6, 30, 0.5, np.float64)
    assert len(hist) - 1 == 8 and hist[1] <= 0.5 * hist[0]
    x, hist = hp_chebyshev.chebyshev(rp, col, val, b, None, None, 0.4, 1.6, 5, 0.5, np.float64)
    assert len(hist) - 1 == 5
    x0 = np.arange(n, dtype=np.float64)
    x, hist = hp_chebyshev.chebyshev(rp, col, val, val * x0, x0, None, 0.4, 1.6, 30, 1e-3, np.float64)
    assert len(hist) - 1 == 0 and hist[0] == 0 and np.array_equal(x, x0)
    x, hist = hp_chebyshev.chebyshev(rp, col, val, b, x0, None, 0.4, 1.6, 0, 0.0, np.float64)
    assert len(hist) == 1 and np.array_equal(x, x0)


# ---- options -------------------------------------------------------------------------------------------------

def test_metadata_defaults(schwz):
    m = schwz.Metadata()
    assert (m.symmetric_solver, m.chebyshev_eig_ratio, m.chebyshev_lambda_min, m.chebyshev_lambda_max) == \
        ("cg", 30.0, 0.0, 0.0)


def _code(schwz, settings_kw=None, **metadata_kw):
    from schwz_amd import solver as sv
    return sv._sym_solver_code(schwz.Settings(**(settings_kw or {})), schwz.Metadata(**metadata_kw))


JACOBI = dict(local_precond="block-jacobi", precond_max_block_size=1)


def test_accepted_combinations(schwz):
    c = schwz.capi
    assert (c.SYM_CG, c.SYM_CHEBYSHEV) == (0, 1)
    assert _code(schwz) == c.SYM_CG
    assert _code(schwz, symmetric_solver="chebyshev", local_precond="null") == c.SYM_CHEBYSHEV
    assert _code(schwz, symmetric_solver="chebyshev", **JACOBI) == c.SYM_CHEBYSHEV
    assert _code(schwz, symmetric_solver="chebyshev", chebyshev_eig_ratio=10.0, chebyshev_lambda_max=2.0,
                 **JACOBI) == c.SYM_CHEBYSHEV


def test_cg_leaves_every_existing_path_alone(schwz):
    """"cg" is accepted with every combination the other validators accept, and none of them reads the new fields."""
    from schwz_amd import solver as sv
    c = schwz.capi
    for skw, mkw in ((dict(), dict(local_precond="ilu", par_ilu_sweeps=2, trisolve_sweeps=2)),
                     (dict(), dict(local_precond="isai")),
                     (dict(), dict(local_precond="block-jacobi", precond_max_block_size=8)),
                     (dict(), dict(local_solver_precision="single", **JACOBI)),
                     (dict(local_solver="direct-ginkgo"), dict()),
                     (dict(non_symmetric_matrix=True), dict(non_symmetric_solver="bicgstab"))):
        s, m = schwz.Settings(**skw), schwz.Metadata(**mkw)
        assert sv._sym_solver_code(s, m) == c.SYM_CG
        sv._factor_solver_code(s, m), sv._precond_code(m), sv._precision_code(s, m), sv._nonsym_solver_code(s, m)


def test_the_field_has_no_effect_without_the_symmetric_iterative_solver(schwz):
    """Like restart_iter: a non-symmetric matrix keeps GMRES / BiCGSTAB, a direct local solver its factors."""
    c = schwz.capi
    assert _code(schwz, dict(non_symmetric_matrix=True), symmetric_solver="chebyshev") == c.SYM_CG
    assert _code(schwz, dict(local_solver="direct-ginkgo"), symmetric_solver="chebyshev") == c.SYM_CG
    assert _code(schwz, dict(non_symmetric_matrix=True), symmetric_solver="chebyshev", local_precond="ilu") == c.SYM_CG


@pytest.mark.parametrize("mkw", [dict(local_precond="ilu"), dict(local_precond="isai"),
                                 dict(local_precond="block-jacobi", precond_max_block_size=4),
                                 dict(local_precond="ilu", par_ilu_sweeps=3),
                                 dict(local_solver_precision="single", **JACOBI)])
def test_refused_combinations_are_not_implemented(schwz, mkw):
    with pytest.raises(schwz.NotImplementedSchwz) as e:
        _code(schwz, symmetric_solver="chebyshev", **mkw)
    assert e.value.code == schwz.capi.ERR_NOT_IMPLEMENTED


def test_parilu_options_are_refused(schwz):
    """(with a preconditioner Chebyshev takes, the sweep counts are already refused by the preconditioner check;
    Chebyshev's own check refuses them too)"""
    from schwz_amd import solver as sv
    m = schwz.Metadata(symmetric_solver="chebyshev", trisolve_sweeps=2, **JACOBI)
    with pytest.raises(schwz.NotImplementedSchwz):
        sv._sym_solver_code(schwz.Settings(), m)
    with pytest.raises(schwz.NotImplementedSchwz):
        sv._precond_code(m)


@pytest.mark.parametrize("settings_kw", [dict(), dict(non_symmetric_matrix=True), dict(local_solver="direct-ginkgo")])
@pytest.mark.parametrize("name", ["cheb", "Chebyshev", "CG", "", None, 1])
def test_unknown_solver_name_is_invalid(schwz, name, settings_kw):
    with pytest.raises(schwz.SchwzError) as e:
        _code(schwz, settings_kw, symmetric_solver=name)
    assert e.value.code == schwz.capi.ERR_INVALID
    assert not isinstance(e.value, schwz.NotImplementedSchwz)


@pytest.mark.parametrize("mkw", [dict(chebyshev_eig_ratio=1.0), dict(chebyshev_eig_ratio=float("nan")),
                                 dict(chebyshev_lambda_min=-1.0), dict(chebyshev_lambda_max=float("inf")),
                                 dict(chebyshev_lambda_min=2.0, chebyshev_lambda_max=1.0)])
def test_bad_bounds_are_invalid(schwz, mkw):
    with pytest.raises(schwz.SchwzError) as e:
        _code(schwz, symmetric_solver="chebyshev", **mkw)
    assert e.value.code == schwz.capi.ERR_INVALID


def test_bounds_from_the_metadata(schwz):
    from schwz_amd import solver as sv
    assert sv._cheb_bounds(schwz.Metadata(), 3.0) == (0.1, 3.0)
    assert sv._cheb_bounds(schwz.Metadata(chebyshev_eig_ratio=10.0), 3.0) == (3.0 / 10.0, 3.0)
    assert sv._cheb_bounds(schwz.Metadata(chebyshev_lambda_max=2.0), 3.0) == (2.0 / 30.0, 2.0)
    assert sv._cheb_bounds(schwz.Metadata(chebyshev_lambda_min=0.25), 3.0) == (0.25, 3.0)
    assert sv._cheb_bounds(schwz.Metadata(chebyshev_lambda_min=0.25, chebyshev_lambda_max=1.5), 3.0) == (0.25, 1.5)


@pytest.mark.parametrize("mkw,code", [(dict(symmetric_solver="sor"), "ERR_INVALID"),
                                      (dict(symmetric_solver="chebyshev", local_precond="ilu"), "ERR_NOT_IMPLEMENTED")])
def test_initialize_refuses_before_any_device_call(schwz, mkw, code):
    """The validator runs at the top of initialize(): no matrix is set up, no subdomain created."""
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(4, 4, 4))
    m = schwz.Metadata(num_subdomains=1, **mkw)

    class NoBackend:
        def __getattr__(self, name):
            raise AssertionError("the backend was touched: %s" % name)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(1), backend=NoBackend(), quiet=True)
    with pytest.raises(schwz.SchwzError) as e:
        solver.initialize()
    assert e.value.code == getattr(schwz.capi, code)


# ---- ABI ---------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared(schwz):
    header = open(os.path.join(ROOT, "include", "schwz_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in schwz.capi.SYMBOLS
        assert getattr(schwz.capi.lib, name) is not None
        assert re.search(r"\b(int|void)\s+%s\(" % name, header), name
    declared = set(re.findall(r"\b(schwz_(?:cheb|ras_(?:set_)?(?:sym_solver|cheb_bounds))\w*)\(", header))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    assert int(re.search(r"#define SCHWZ_CHEB_CHECK_EVERY (\d+)", header).group(1)) == schwz.capi.CHEB_CHECK_EVERY == \
        hp_chebyshev.CHECK_EVERY
    assert re.search(r"enum schwz_sym_solver \{ SCHWZ_SYM_CG = 0, SCHWZ_SYM_CHEBYSHEV = 1 \}", header)


def test_capi_refuses_before_touching_the_matrix(schwz):
    """schwz_cheb_create checks the preconditioner code and the output pointer before it looks at the matrix, as
    schwz_pcg_f32_create does."""
    lib, c = schwz.capi.lib, schwz.capi
    h = ctypes.c_void_p()
    create = lib.schwz_cheb_create
    for pc in (c.PRECOND_BLOCK_JACOBI, c.PRECOND_ILU, c.PRECOND_ISAI):
        assert create(None, pc, ctypes.byref(h)) == c.ERR_NOT_IMPLEMENTED
        assert not h.value
    for pc in (99, -1, 5):
        assert create(None, pc, ctypes.byref(h)) == c.ERR_INVALID
    assert create(None, c.PRECOND_JACOBI, None) == c.ERR_INVALID              # null output pointer
    assert create(None, c.PRECOND_JACOBI, ctypes.byref(h)) == c.ERR_INVALID   # ... and only then the null matrix
    assert create(None, c.PRECOND_ILU, None) == c.ERR_INVALID
    for pc in (c.PRECOND_BLOCK_JACOBI, 99):
        assert create(None, pc, ctypes.byref(h)) == lib.schwz_pcg_f32_create(None, pc, ctypes.byref(h))
    lib.schwz_cheb_destroy(None)
    lo, hi = ctypes.c_double(0.0), ctypes.c_double(0.0)
    assert lib.schwz_cheb_bounds(None, ctypes.byref(lo), ctypes.byref(hi)) == c.ERR_INVALID
    assert lib.schwz_cheb_set_bounds(None, 0.1, 1.0) == c.ERR_INVALID
    # no subdomain: CG, and nothing to set
    assert lib.schwz_ras_sym_solver(None) == c.SYM_CG
    assert lib.schwz_ras_set_sym_solver(None, c.SYM_CHEBYSHEV) == c.ERR_INVALID
    assert lib.schwz_ras_set_sym_solver(None, 7) == c.ERR_INVALID
    assert lib.schwz_ras_cheb_bounds(None, ctypes.byref(lo), ctypes.byref(hi)) == c.ERR_INVALID
    assert lib.schwz_ras_set_cheb_bounds(None, 0.1, 1.0) == c.ERR_INVALID


def test_set_bounds_checks_its_values(schwz):
    """0 < lmin < lmax, both finite; the values are checked before the solver is looked at."""
    lib, c = schwz.capi.lib, schwz.capi
    nan, inf = float("nan"), float("inf")
    for lo, hi in ((0.0, 1.0), (-0.5, 1.0), (1.0, 1.0), (2.0, 1.0), (nan, 1.0), (0.1, nan), (0.1, inf), (inf, inf),
                   (-inf, 1.0)):
        assert lib.schwz_cheb_set_bounds(None, lo, hi) == c.ERR_INVALID
        assert "0 < lmin < lmax" in lib.schwz_last_error().decode()
    assert lib.schwz_cheb_set_bounds(None, 0.1, 1.0) == c.ERR_INVALID
    assert "null solver" in lib.schwz_last_error().decode()


def test_setter_needs_a_subdomain_on_the_device(schwz):
    p = schwz.Problem.laplacian(2, 8)
    sd = schwz.Subdomain(p, 1, 0, 2, schwz.partition_regular(64, 1))
    with pytest.raises(schwz.SchwzError) as e:
        sd.set_sym_solver(schwz.capi.SYM_CHEBYSHEV)
    assert e.value.code == schwz.capi.ERR_INVALID
    with pytest.raises(schwz.SchwzError) as e:
        sd.set_sym_solver(5)
    assert e.value.code == schwz.capi.ERR_INVALID
    with pytest.raises(schwz.SchwzError) as e:
        sd.cheb_bounds()
    assert e.value.code == schwz.capi.ERR_INVALID
    assert sd.sym_solver() == schwz.capi.SYM_CG


def test_solver_options_are_unchanged(schwz):
    """The choice travels through schwz_ras_set_sym_solver: the options struct keeps its layout."""
    assert [n for n, _ in schwz.capi.SolverOptions._fields_] == [
        "local_solver", "precond", "local_tol", "local_max_iters", "natural_factor_ordering", "spmv_variant",
        "precond_block_size", "non_symmetric", "restart_iter", "par_ilu_sweeps", "trisolve_sweeps"]
    assert ctypes.sizeof(schwz.capi.SolverOptions) == 48
