"""Compressed-basis GMRES (Metadata.gmres_basis, schwz_gmres_create_basis, schwz_ras_set_gmres_basis): the default,
what the host accepts and refuses before any device call, the cases where the field has no effect, the argument
checks of the C ABI that need no GPU, the field of the C++ mirror, and the restatement of tests/hp_gmres_cb.py pinned
by the fp64 restatement of hp_reference and by cases that can be checked by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import hp_gmres_cb
import hp_reference as hp
from conftest import convection_diffusion_2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_metadata_field_defaults_to_double(schwz):
    assert schwz.Metadata().gmres_basis == "double"


def _code(schwz, settings_kw=None, **metadata_kw):
    from schwz_amd import solver as sv
    return sv._gmres_basis_code(schwz.Settings(**(settings_kw or {})), schwz.Metadata(**metadata_kw))


def test_accepted_combinations(schwz):
    c = schwz.capi
    assert (c.GMRES_BASIS_F64, c.GMRES_BASIS_F32) == (0, 1)
    nonsym = dict(non_symmetric_matrix=True)
    assert _code(schwz) == c.GMRES_BASIS_F64
    assert _code(schwz, nonsym) == c.GMRES_BASIS_F64
    assert _code(schwz, nonsym, gmres_basis="double") == c.GMRES_BASIS_F64
    assert _code(schwz, nonsym, gmres_basis="single") == c.GMRES_BASIS_F32
    assert _code(schwz, nonsym, gmres_basis="single", non_symmetric_solver="gmres") == c.GMRES_BASIS_F32
    # every preconditioner and the ParILU options: the basis type does not touch them
    for pc in (dict(local_precond="null"), dict(local_precond="block-jacobi", precond_max_block_size=1),
               dict(local_precond="block-jacobi", precond_max_block_size=8), dict(local_precond="ilu"),
               dict(local_precond="isai"), dict(local_precond="ilu", par_ilu_sweeps=3, trisolve_sweeps=2)):
        assert _code(schwz, nonsym, gmres_basis="single", **pc) == c.GMRES_BASIS_F32
    for restart in (1, 8, 9, 30, 2048):
        assert _code(schwz, dict(non_symmetric_matrix=True, restart_iter=restart),
                     gmres_basis="single") == c.GMRES_BASIS_F32


def test_the_field_has_no_effect_where_gmres_does_not_run(schwz):
    """Like restart_iter: a symmetric matrix keeps its CG, a direct local solver its factors, BiCGSTAB its vectors."""
    c = schwz.capi
    assert _code(schwz, gmres_basis="single") == c.GMRES_BASIS_F64
    assert _code(schwz, dict(local_solver="direct-ginkgo"), gmres_basis="single") == c.GMRES_BASIS_F64
    assert _code(schwz, dict(non_symmetric_matrix=True, local_solver="direct-ginkgo", factorization="umfpack"),
                 gmres_basis="single") == c.GMRES_BASIS_F64
    assert _code(schwz, dict(non_symmetric_matrix=True), gmres_basis="single",
                 non_symmetric_solver="bicgstab") == c.GMRES_BASIS_F64


@pytest.mark.parametrize("settings_kw", [dict(), dict(non_symmetric_matrix=True), dict(local_solver="direct-ginkgo")])
@pytest.mark.parametrize("name", ["half", "Single", "float", "fp32", "", None, 1])
def test_unknown_basis_name_is_invalid(schwz, name, settings_kw):
    with pytest.raises(schwz.SchwzError) as e:
        _code(schwz, settings_kw, gmres_basis=name)
    assert e.value.code == schwz.capi.ERR_INVALID
    assert not isinstance(e.value, schwz.NotImplementedSchwz)


def test_initialize_refuses_before_any_device_call(schwz):
    """The validator runs at the top of initialize(): no matrix is set up, no subdomain created."""
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(4, 4, 4), non_symmetric_matrix=True)
    m = schwz.Metadata(num_subdomains=1, gmres_basis="float")

    class NoBackend:
        def __getattr__(self, name):
            raise AssertionError("the backend was touched: %s" % name)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(1), backend=NoBackend(), quiet=True)
    with pytest.raises(schwz.SchwzError) as e:
        solver.initialize()
    assert e.value.code == schwz.capi.ERR_INVALID


def test_single_precision_local_solve_still_refused_and_points_to_the_basis(schwz):
    from schwz_amd import solver as sv
    with pytest.raises(schwz.NotImplementedSchwz) as e:
        sv._precision_code(schwz.Settings(non_symmetric_matrix=True), schwz.Metadata(local_solver_precision="single"))
    assert e.value.code == schwz.capi.ERR_NOT_IMPLEMENTED
    assert "gmres_basis" in str(e.value)
    # ... also when the compressed basis is asked for as well
    with pytest.raises(schwz.NotImplementedSchwz):
        sv._precision_code(schwz.Settings(non_symmetric_matrix=True),
                           schwz.Metadata(local_solver_precision="single", gmres_basis="single"))


def test_capi_refuses_before_touching_the_matrix(schwz):
    """schwz_gmres_create_basis refuses an unknown basis code first, then runs the checks of schwz_gmres_create_ex."""
    lib, c = schwz.capi.lib, schwz.capi
    h = ctypes.c_void_p()
    create = lib.schwz_gmres_create_basis
    for basis in (2, -1, 7):
        assert create(None, c.PRECOND_JACOBI, 1, 4, 0, 0, basis, ctypes.byref(h)) == c.ERR_INVALID
        assert not h.value
    for basis in (c.GMRES_BASIS_F64, c.GMRES_BASIS_F32):
        for args in ((c.PRECOND_JACOBI, 1, 0, 0), (99, 1, 0, 0), (c.PRECOND_ILU, 1, -1, 0),
                     (c.PRECOND_JACOBI, 1, 2, 0), (c.PRECOND_ISAI, 1, 0, 3)):
            want = lib.schwz_gmres_create_ex(None, args[0], args[1], 4, args[2], args[3], ctypes.byref(h))
            assert want != c.OK
            assert create(None, args[0], args[1], 4, args[2], args[3], basis, ctypes.byref(h)) == want, args
            assert not h.value
        assert create(None, c.PRECOND_JACOBI, 1, 4, 0, 0, basis, None) == c.ERR_INVALID
    assert lib.schwz_gmres_basis(None) == c.GMRES_BASIS_F64
    # no subdomain: fp64, and nothing to set
    assert lib.schwz_ras_gmres_basis(None) == c.GMRES_BASIS_F64
    assert lib.schwz_ras_set_gmres_basis(None, c.GMRES_BASIS_F32) == c.ERR_INVALID
    assert lib.schwz_ras_set_gmres_basis(None, 7) == c.ERR_INVALID


def test_setter_needs_a_subdomain_on_the_device(schwz):
    p = schwz.Problem.laplacian(2, 8)
    sd = schwz.Subdomain(p, 1, 0, 2, schwz.partition_regular(64, 1))
    with pytest.raises(schwz.SchwzError) as e:
        sd.set_gmres_basis(schwz.capi.GMRES_BASIS_F32)
    assert e.value.code == schwz.capi.ERR_INVALID
    with pytest.raises(schwz.SchwzError) as e:
        sd.set_gmres_basis(5)
    assert e.value.code == schwz.capi.ERR_INVALID
    assert sd.gmres_basis() == schwz.capi.GMRES_BASIS_F64


def test_solver_options_are_unchanged(schwz):
    """The choice travels through schwz_ras_set_gmres_basis: the options struct keeps its layout."""
    assert ctypes.sizeof(schwz.capi.SolverOptions) == 48


def test_header_and_binding_agree(schwz):
    header = open(os.path.join(ROOT, "include", "schwz_hip.h")).read()
    mt = re.search(r"enum schwz_gmres_basis \{ SCHWZ_GMRES_BASIS_F64 = (\d+), SCHWZ_GMRES_BASIS_F32 = (\d+) \};", header)
    assert mt and (int(mt.group(1)), int(mt.group(2))) == (schwz.capi.GMRES_BASIS_F64, schwz.capi.GMRES_BASIS_F32)
    for name in ("schwz_gmres_create_basis", "schwz_gmres_basis", "schwz_ras_set_gmres_basis", "schwz_ras_gmres_basis"):
        assert name in schwz.capi.SYMBOLS and re.search(r"\b%s\(" % name, header)
    # the caveat on the recurred norm is part of the contract
    assert "RECURRED" in header and "2^-24" in header


def test_mirror_has_the_field_with_the_same_rules():
    """The C++ mirror: the field and its default in settings.hpp, the name check and the no-effect cases in
    initialize() (the run through the mirror is tests/test_gpu_gmres_basis.py)."""
    host = os.path.join(ROOT, "schwarz-lib_amd", "host")
    settings = open(os.path.join(host, "include", "settings.hpp")).read()
    assert re.search(r'std::string gmres_basis = "double";', settings)
    base = open(os.path.join(host, "src", "schwarz_base.cpp")).read()
    assert re.search(r'm\.gmres_basis != "double" && m\.gmres_basis != "single"', base)
    mt = re.search(r"const bool f32_basis = ([^;]+);", base)
    assert mt
    rule = mt.group(1)
    assert "non_symmetric_matrix" in rule and "SCHWZ_SOLVER_ITERATIVE" in rule and "!bicgstab_local" in rule
    assert "schwz_ras_set_gmres_basis(im.sd, SCHWZ_GMRES_BASIS_F32)" in base


def test_iteration_spread_of_the_restatements():
    """The allowance of the device tests on the iteration count is one plus the largest difference between the
    float64 and the longdouble restatement over their cases (gmres_cb_cases.SPREAD): measured here."""
    import gmres_cb_cases as cc
    spread = max(abs(cc.ref(case).iters64 - cc.ref(case).iters) for case in cc.SMALL)
    print("spread of the iteration counts over %d cases: %d" % (len(cc.SMALL), spread))
    assert spread == cc.SPREAD


# ---- the restatement ---------------------------------------------------------------------------------------

def _tridiag(n, lo=-1.3, d=2.5, up=-0.7):
    import scipy.sparse as sp
    a = sp.diags([np.full(max(n - 1, 0), lo), np.full(n, d), np.full(max(n - 1, 0), up)], [-1, 0, 1], shape=(n, n),
                 format="csr")
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


@pytest.mark.parametrize("dtype", [np.float64, hp.LD])
@pytest.mark.parametrize("m", [1, 9, 30])
def test_restatement_without_rounding_is_gmres(dtype, m):
    """The same text with the rounding switched off is GMRES with CGS2 in place of MGS: the iterates of
    hp_reference.gmres to rounding, and its iteration count."""
    rp, col, val = convection_diffusion_2d(12)
    n = len(rp) - 1
    b = np.random.default_rng(3).standard_normal(n)
    M = hp.precond_jacobi(rp, col, val, dtype)
    x_ref, h_ref = hp.gmres(rp, col, val, b, None, M, 400, m, 1e-9, dtype)
    x, h = hp_gmres_cb.gmres_cb(rp, col, val, b, None, M, 400, m, 1e-9, dtype, round_basis=False)
    assert len(h) == len(h_ref)
    assert np.abs(x - x_ref).max() <= 1e-10 * np.abs(x_ref).max()


@pytest.mark.parametrize("m", [10, 30])
def test_restarted_counts_are_those_of_the_fp64_basis(m):
    """What the method promises: with restarts the rounding of the basis costs no iterations (a count within one of
    the fp64 basis'), and the true residual is within hp_gmres_cb.cycle_bound, slack 1 % for the fp64 rounding of
    everything else."""
    rp, col, val = convection_diffusion_2d(24)
    n = len(rp) - 1
    b = np.random.default_rng(5).standard_normal(n)
    M = hp.precond_jacobi(rp, col, val, np.float64)
    for rtol in (1e-6, 1e-10):
        _, h_ref = hp.gmres(rp, col, val, b, None, M, 4000, m, rtol, np.float64)
        cyc = []
        x, h = hp_gmres_cb.gmres_cb(rp, col, val, b, None, M, 4000, m, rtol, np.float64, cycle_starts=cyc)
        true = hp_gmres_cb.true_relres(rp, col, val, x, b)
        print("m = %d, rtol %.0e: %d iterations, fp64 basis %d; true relres %.3e, bound %.3e" %
              (m, rtol, len(h) - 1, len(h_ref) - 1, true, hp_gmres_cb.cycle_bound(h, cyc)))
        assert abs((len(h) - 1) - (len(h_ref) - 1)) <= 1
        assert h[-1] <= rtol * h[0]
        assert true <= 1.01 * hp_gmres_cb.cycle_bound(h, cyc)


def test_one_long_cycle_stops_on_the_recurred_norm():
    """The documented cost: inside ONE cycle the true residual follows the recurred norm only to about 2^-24 of the
    cycle's start residual.  A 1e-10 reduction without a restart stops on the recurred norm; the true residual is
    within cycle_bound (about 6e-8 here), and a second, warm-started solve -- whose start residual is recomputed in
    fp64, as every restart and every outer iteration does -- brings it to 1e-10 of the first start residual."""
    rp, col, val = convection_diffusion_2d(16)
    n = len(rp) - 1
    b = np.random.default_rng(7).standard_normal(n)
    M = hp.precond_jacobi(rp, col, val, np.float64)
    cyc = []
    x, h = hp_gmres_cb.gmres_cb(rp, col, val, b, None, M, n, n, 1e-10, np.float64, cycle_starts=cyc)
    assert len(cyc) == 1 and h[-1] <= 1e-10 * h[0]
    true = hp_gmres_cb.true_relres(rp, col, val, x, b)
    print("one cycle of %d vectors: recurred %.3e, true %.3e" % (len(h) - 1, h[-1] / h[0], true))
    assert true <= 1.01 * hp_gmres_cb.cycle_bound(h, cyc)
    assert hp_gmres_cb.cycle_bound(h, cyc) <= 1e-10 + 2.0 ** -24
    x2, h2 = hp_gmres_cb.gmres_cb(rp, col, val, b, x, M, n, n, 1e-10 * h[0] / max(true * h[0], 1e-300), np.float64)
    assert hp_gmres_cb.true_relres(rp, col, val, x2, b) <= 1.01 * (1e-10 + 2.0 ** -24 * true)


@pytest.mark.parametrize("dtype", [np.float64, hp.LD])
def test_restatement_by_hand(dtype):
    none = hp.precond_none(dtype)
    # A = I and a right-hand side whose normalisation fp32 holds exactly: v_0 = b / 4, w = v_0, h = 1, w - h v_0 = 0
    # exactly, eta = 0, the rotation is the identity, resn = 0: one Krylov vector and x = b
    n = 16
    rp, col, val = np.arange(n + 1), np.arange(n), np.ones(n)
    b = np.random.default_rng(1).choice([-1.0, 1.0], n)
    x, h = hp_gmres_cb.gmres_cb(rp, col, val, b, None, none, 5, 3, 0.0, dtype)
    assert len(h) - 1 == 1 and h[-1] == 0
    assert np.array_equal(np.asarray(x, dtype=np.float64), b)
    # b = 0: nothing runs
    x, h = hp_gmres_cb.gmres_cb(rp, col, val, np.zeros(n), None, none, 5, 3, 1e-8, dtype)
    assert len(h) == 1 and h[0] == 0 and not np.asarray(x).any()
    # max_iters = 0
    rp, col, val = _tridiag(9)
    x0 = np.arange(9, dtype=np.float64) - 4
    x, h = hp_gmres_cb.gmres_cb(rp, col, val, np.ones(9), x0, none, 0, 4, 1e-8, dtype)
    assert len(h) == 1 and h[0] > 0
    assert np.array_equal(np.asarray(x, dtype=np.float64), x0)
    # max_iters not a multiple of the restart length: 4 + 3 vectors
    x, h = hp_gmres_cb.gmres_cb(rp, col, val, np.ones(9), x0, none, 7, 4, 0.0, dtype)
    assert len(h) - 1 == 7
    # the two rounding points: every stored basis vector is an fp32 vector (seen through the restatement's result:
    # with one Krylov vector x - x0 is a multiple of fl32(r / beta))
    b = np.random.default_rng(2).standard_normal(9)
    x, h = hp_gmres_cb.gmres_cb(rp, col, val, b, None, none, 1, 1, 0.0, dtype)
    v0 = hp_gmres_cb.fl32(np.asarray(b, dtype=dtype) / np.sqrt(hp.dot(np.asarray(b, dtype=dtype), np.asarray(b, dtype=dtype))), dtype)
    k = int(np.argmax(np.abs(v0)))
    assert np.abs(x / (x[k] / v0[k]) - v0).max() <= 8 * np.finfo(dtype).eps
