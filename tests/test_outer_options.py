"""The outer FGMRES: what of it can be checked without a GPU -- the two Metadata fields, the refusals (all raised before
any device allocation: the backend and the subdomains of these solvers fail at the first touch), the ABI surface, the
argument checks of the library and the host Givens / least-squares code.  Pattern: tests/test_batch_options.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["schwz_ras_apply_interior", "schwz_outer_create", "schwz_outer_destroy", "schwz_outer_vector",
               "schwz_outer_start", "schwz_outer_dots", "schwz_outer_project_dots", "schwz_outer_normalize",
               "schwz_outer_combine", "schwz_outer_copy"]
N = 12


class NoBackend:
    """Any use of the backend is a device call made too early."""

    def __getattr__(self, name):
        raise AssertionError("the backend was touched: %s" % name)


class NoSubdomain:
    def __getattr__(self, name):
        raise AssertionError("a subdomain was touched: %s" % name)


class TwoProcessComm:
    """What the checks read of a communicator of two rank processes, one subdomain each."""
    size, rank, local_ranks, is_root = 2, 0, [0], True


def _solver(schwz, set_up=True, settings=None, comm_settings=None, comm=None, **metadata):
    s = schwz.Settings(**(settings or {}))
    for k, v in (comm_settings or {}).items():
        setattr(s.comm_settings, k, v)
    m = schwz.Metadata(num_subdomains=1, **metadata)
    solver = schwz.SolverRAS(s, m, comm=comm or schwz.InProcessComm(1), backend=NoBackend(), quiet=True)
    if set_up:  # what initialize() leaves, as far as the checks look
        solver.problem = object()
        solver.subdomains = {0: NoSubdomain()}
        m.global_size = N
    return solver


def _invalid(schwz, call):
    with pytest.raises(schwz.SchwzError) as e:
        call()
    assert e.value.code == schwz.capi.ERR_INVALID, e.value
    assert not isinstance(e.value, schwz.NotImplementedSchwz)
    return str(e.value)


def test_field_defaults(schwz):
    m = schwz.Metadata()
    assert m.outer_iteration == "richardson" and m.outer_restart == 30
    from schwz_amd import outer
    assert outer.wants_fgmres(schwz.Settings(), m, schwz.InProcessComm(1)) is False
    m.outer_iteration = "fgmres"
    assert outer.wants_fgmres(schwz.Settings(), m, schwz.InProcessComm(1)) is True


@pytest.mark.parametrize("name", ["gmres", "FGMRES", "", "anderson", None, 1])
def test_unknown_outer_iterations_are_invalid(schwz, name):
    for set_up in (True, False):
        solver = _solver(schwz, set_up=set_up, outer_iteration=name)
        assert "outer_iteration" in _invalid(schwz, solver.run)
        assert "outer_iteration" in _invalid(schwz, solver.initialize)


@pytest.mark.parametrize("restart", [0, -1, -30, 129, 2.5, None, "30", True])
@pytest.mark.parametrize("name", ["richardson", "fgmres"])
def test_outer_restart_out_of_range_is_invalid(schwz, name, restart):
    solver = _solver(schwz, outer_iteration=name, outer_restart=restart)
    assert "outer_restart" in _invalid(schwz, solver.run)
    assert "outer_restart" in _invalid(schwz, solver.initialize)


REFUSED = {
    "coarse space": dict(coarse_space="aggregates", coarse_aggregates=4),
    "onesided": dict(comm_settings=dict(enable_onesided=True)),
    "overlap": dict(comm_settings=dict(enable_overlap=True)),
    "onesided + overlap": dict(comm_settings=dict(enable_onesided=True, enable_overlap=True)),
    "fp32 halos": dict(settings=dict(use_mixed_precision=True)),
    "two-stage": dict(settings=dict(reset_local_crit_iter=4)),
    "two rank processes": dict(comm=TwoProcessComm()),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_configurations_without_the_loop_are_not_implemented(schwz, name):
    """NotImplemented from run(), solve() and initialize(), on a set-up solver and on one that is not, before the
    backend or a subdomain is touched; the same configuration with the default outer iteration is not refused here."""
    from schwz_amd import outer
    for set_up in (True, False):
        solver = _solver(schwz, set_up=set_up, outer_iteration="fgmres", **REFUSED[name])
        for call in (solver.run, solver.initialize):
            with pytest.raises(schwz.NotImplementedSchwz) as e:
                call()
            assert e.value.code == schwz.capi.ERR_NOT_IMPLEMENTED and "fgmres" in str(e.value)
    solver = _solver(schwz, **REFUSED[name])
    assert outer.wants_fgmres(solver.settings, solver.metadata, solver.comm) is False


@pytest.mark.parametrize("config", [
    dict(settings=dict(local_solver="direct-cholmod")),
    dict(settings=dict(local_solver="direct-ginkgo", factorization="umfpack", non_symmetric_matrix=True)),
    dict(settings=dict(non_symmetric_matrix=True), non_symmetric_solver="bicgstab"),
    dict(settings=dict(non_symmetric_matrix=True), gmres_basis="single"),
    dict(symmetric_solver="chebyshev", local_precond="block-jacobi", precond_max_block_size=1),
    dict(local_solver_precision="single"), dict(local_precond="ilu", par_ilu_sweeps=2), dict(local_precond="isai"),
], ids=["cholmod", "umfpack", "bicgstab", "fp32 basis", "chebyshev", "fp32 cg", "parilu", "isai"])
def test_every_local_solver_is_allowed(schwz, config):
    from schwz_amd import outer
    solver = _solver(schwz, outer_iteration="fgmres", outer_restart=5, **config)
    assert outer.wants_fgmres(solver.settings, solver.metadata, solver.comm) is True


def test_refused_before_initialize(schwz):
    solver = _solver(schwz, set_up=False, outer_iteration="fgmres")
    assert "initialize" in _invalid(schwz, solver.run)


def test_solve_many_ignores_the_field(schwz):
    """The block path looks at its own refusals only: a bad right-hand side is what it complains about."""
    solver = _solver(schwz, outer_iteration="fgmres", local_precond="block-jacobi", precond_max_block_size=1)
    assert "shape" in _invalid(schwz, lambda: solver.solve_many(np.ones(N)))


def test_new_symbols_are_exported_declared_and_listed(schwz):
    header = open(os.path.join(ROOT, "include", "schwz_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in schwz.capi.SYMBOLS
        assert getattr(schwz.capi.lib, name) is not None
        assert re.search(r"\b(int|void)\s+%s\(" % name, header), name
    declared = set(re.findall(r"\b(schwz_(?:outer_|ras_apply_interior)\w*)\(", header))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    assert callable(schwz.Subdomain.apply_interior) and callable(schwz.Outer.project_dots) and callable(schwz.outer_copy)


def test_capi_refuses_null_and_out_of_range_arguments(schwz):
    """SCHWZ_ERR_INVALID before any HIP call (this test runs without a GPU), and a refused call writes nothing."""
    lib, c = schwz.capi.lib, schwz.capi
    one, out = np.ones(64), np.full(8, 7.0)
    h, p = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.schwz_outer_create(16, 5, None) == c.ERR_INVALID
    for n, restart in ((-1, 5), (16, 0), (16, -3), (16, 129)):
        assert lib.schwz_outer_create(n, restart, ctypes.byref(h)) == c.ERR_INVALID and not h.value
    assert lib.schwz_outer_vector(None, 0, 0, ctypes.byref(p)) == c.ERR_INVALID and not p.value
    assert lib.schwz_outer_start(None, 1.0, None) == c.ERR_INVALID
    assert lib.schwz_outer_dots(None, 0, c.ptr(out), None) == c.ERR_INVALID
    assert lib.schwz_outer_project_dots(None, 0, c.ptr(one), c.ptr(out), None) == c.ERR_INVALID
    assert lib.schwz_outer_normalize(None, 0, 1.0, None) == c.ERR_INVALID
    assert lib.schwz_outer_combine(None, 1, c.ptr(one), c.ptr(one), None) == c.ERR_INVALID
    assert lib.schwz_outer_copy(-1, c.ptr(one), c.ptr(one), None) == c.ERR_INVALID
    assert lib.schwz_outer_copy(4, None, c.ptr(one), None) == c.ERR_INVALID
    assert lib.schwz_outer_copy(4, c.ptr(one), None, None) == c.ERR_INVALID
    lib.schwz_outer_destroy(None)
    sd = schwz.Subdomain(schwz.Problem.laplacian(2, 8), 1, 0, 2, schwz.partition_regular(64, 1))
    for s in (None, sd.h):
        assert lib.schwz_ras_apply_interior(s, c.ptr(one), None) == c.ERR_INVALID
        assert b"not on the device" in lib.schwz_last_error()
    assert list(out) == [7.0] * 8 and list(one) == [1.0] * 64


@pytest.mark.parametrize("m", [1, 2, 5, 30])
@pytest.mark.parametrize("seed", [0, 1])
def test_givens_least_squares_against_lstsq(m, seed):
    """Random (m + 1) x m upper Hessenberg matrices, column by column: the residual norm after every column and the
    solution against numpy.linalg.lstsq on the leading blocks."""
    from schwz_amd.outer import GivensLeastSquares
    rng = np.random.default_rng(seed)
    H = np.triu(rng.standard_normal((m + 1, m)), -1)
    H[np.arange(1, m + 1), np.arange(m)] = np.abs(H[np.arange(1, m + 1), np.arange(m)]) + 0.1
    beta = 3.5
    ls = GivensLeastSquares(m, beta)
    for k in range(m):
        est = ls.append(H[:k + 2, k])
        rhs = np.zeros(k + 2)
        rhs[0] = beta
        y_ref, *_ = np.linalg.lstsq(H[:k + 2, :k + 1], rhs, rcond=None)
        res_ref = np.linalg.norm(rhs - H[:k + 2, :k + 1] @ y_ref)
        cond = np.linalg.cond(H[:k + 2, :k + 1])
        assert abs(est - res_ref) <= 1e-13 * beta * max(cond, 1.0)
        y = ls.solve()
        assert np.abs(y - y_ref).max() <= 1e-13 * cond * max(np.abs(y_ref).max(), 1.0)


def test_givens_least_squares_breakdown():
    """h_{j+1,j} = 0 ends the cycle cleanly: the residual of the least-squares problem is zero and the solve is exact."""
    from schwz_amd.outer import GivensLeastSquares
    ls = GivensLeastSquares(3, 2.0)
    assert ls.append([4.0, 3.0]) == pytest.approx(2.0 * 3.0 / 5.0)
    assert ls.append([1.0, 2.0, 0.0]) == 0.0
    H = np.array([[4.0, 1.0], [3.0, 2.0]])
    assert np.allclose(H @ ls.solve(), [2.0, 0.0], atol=1e-15)
