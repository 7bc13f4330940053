"""A block of right-hand sides at once: what of SolverRAS.solve_many and of the block entry points can be checked
without a GPU -- the refusals (all raised before any device allocation: the backend and the subdomains of these solvers
fail at the first touch), the padding arithmetic of the blocks, the ABI surface and the argument checks of the
library.  Pattern: tests/test_resolve_options.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["schwz_csr_spmm", "schwz_bcg_create", "schwz_bcg_destroy", "schwz_bcg_solve", "schwz_bcg_last_stats",
               "schwz_bcg_residual", "schwz_ras_batch_begin", "schwz_ras_batch_end", "schwz_ras_batch_rhs_set",
               "schwz_ras_batch_pack", "schwz_ras_batch_unpack", "schwz_ras_batch_update_boundary",
               "schwz_ras_batch_local_residual", "schwz_ras_batch_local_solve", "schwz_ras_batch_restrict",
               "schwz_ras_batch_vector", "schwz_ras_batch_get_interior", "schwz_ras_batch_true_residual_sq"]
N = 12


class NoBackend:
    """Any use of the backend is a device call made too early."""

    def __getattr__(self, name):
        raise AssertionError("the backend was touched: %s" % name)


class NoSubdomain:
    def __getattr__(self, name):
        raise AssertionError("a subdomain was touched: %s" % name)


def _solver(schwz, set_up=True, settings=None, comm_settings=None, **metadata):
    s = schwz.Settings(**(settings or {}))
    for k, v in (comm_settings or {}).items():
        setattr(s.comm_settings, k, v)
    m = schwz.Metadata(num_subdomains=1, **dict(dict(local_precond="block-jacobi", precond_max_block_size=1), **metadata))
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(1), backend=NoBackend(), quiet=True)
    if set_up:  # what initialize() leaves, as far as the checks look: a problem, subdomains, the global size
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


UNAVAILABLE = {
    "non_symmetric_matrix": dict(settings=dict(non_symmetric_matrix=True)),
    "direct local solver": dict(settings=dict(local_solver="direct-ginkgo")),
    "direct-cholmod": dict(settings=dict(local_solver="direct-cholmod")),
    "block-jacobi 4": dict(precond_max_block_size=4),
    "ilu": dict(local_precond="ilu"),
    "isai": dict(local_precond="isai"),
    "single precision": dict(local_solver_precision="single"),
    "chebyshev": dict(symmetric_solver="chebyshev"),
    "coarse space": dict(coarse_space="aggregates", coarse_aggregates=4),
    "onesided": dict(comm_settings=dict(enable_onesided=True)),
    "fp32 halos": dict(settings=dict(use_mixed_precision=True)),
    "two-stage": dict(settings=dict(reset_local_crit_iter=4)),
    "par_ilu_sweeps": dict(local_precond="ilu", par_ilu_sweeps=3),
    "trisolve_sweeps": dict(local_precond="ilu", trisolve_sweeps=2),
}


@pytest.mark.parametrize("name", sorted(UNAVAILABLE))
def test_configurations_without_a_block_path_are_not_implemented(schwz, name):
    """NotImplemented, on a set-up solver and on one that is not (the configuration is looked at first), and before
    the right-hand sides are looked at."""
    for set_up in (True, False):
        solver = _solver(schwz, set_up=set_up, **UNAVAILABLE[name])
        for rhs in (np.ones((N, 3)), np.ones(N), None):
            with pytest.raises(schwz.NotImplementedSchwz) as e:
                solver.solve_many(rhs)
            assert e.value.code == schwz.capi.ERR_NOT_IMPLEMENTED


@pytest.mark.parametrize("precond", [dict(local_precond="null"), dict(local_precond="block-jacobi", precond_max_block_size=1)])
def test_the_two_preconditioners_with_a_block_path_pass_the_configuration_check(schwz, precond):
    solver = _solver(schwz, **precond)
    assert solver._check_batch(np.ones((N, 3))).shape == (N, 3)


def test_refused_before_initialize(schwz):
    solver = _solver(schwz, set_up=False)
    assert "initialize" in _invalid(schwz, lambda: solver.solve_many(np.ones((N, 2))))


@pytest.mark.parametrize("bad", [
    np.ones(N), np.ones((N - 1, 2)), np.ones((N + 1, 2)), np.ones((2, N)), np.ones((N, 2, 1)), np.float64(1.0),   # shape
    np.ones((N, 0)),                                                                                              # nrhs < 1
    np.ones((N, 2), dtype=np.int64), np.ones((N, 2), dtype=bool), np.ones((N, 2), dtype=np.complex128),           # not floats
    [["a", "b"]] * N,
    np.r_[np.ones(2 * N - 1), np.nan].reshape(N, 2), np.r_[np.inf, np.ones(2 * N - 1)].reshape(N, 2),            # not finite
    np.r_[np.ones(2 * N - 1), -np.inf].reshape(N, 2),
], ids=["vector", "short", "long", "transposed", "rank3", "scalar", "no columns", "int64", "bool", "complex", "strings",
        "nan", "inf", "-inf"])
def test_host_arrays_refused(schwz, bad):
    solver = _solver(schwz)
    _invalid(schwz, lambda: solver.solve_many(bad))


def test_a_tensor_is_refused(schwz):
    import torch
    solver = _solver(schwz)
    _invalid(schwz, lambda: solver.solve_many(torch.ones((N, 2), dtype=torch.float64)))


@pytest.mark.parametrize("nrhs,blocks", [(1, (2,)), (2, (2,)), (3, (4,)), (4, (4,)), (5, (8,)), (7, (8,)), (8, (8,)),
                                         (9, (8, 2)), (12, (8, 4)), (13, (8, 8)), (16, (8, 8)), (17, (8, 8, 2))])
def test_padding_arithmetic(schwz, nrhs, blocks):
    """Blocks of 8, the last one padded up to 2, 4 or 8."""
    assert schwz.batch_blocks(nrhs) == blocks
    assert all(k in schwz.capi.BATCH_WIDTHS for k in blocks) and sum(blocks) >= nrhs > sum(blocks) - blocks[-1]


@pytest.mark.parametrize("nrhs", [0, -1])
def test_fewer_than_one_column_is_refused(schwz, nrhs):
    _invalid(schwz, lambda: schwz.batch_blocks(nrhs))


def test_new_symbols_are_exported_declared_and_listed(schwz):
    header = open(os.path.join(ROOT, "include", "schwz_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in schwz.capi.SYMBOLS
        assert getattr(schwz.capi.lib, name) is not None
        assert re.search(r"\b(int|void)\s+%s\(" % name, header), name
    declared = set(re.findall(r"\b(schwz_(?:csr_spmm|bcg_|ras_batch_)\w*)\(", header))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    for name in ("batch_begin", "batch_end", "batch_rhs_set", "batch_pack", "batch_unpack", "batch_update_boundary",
                 "batch_local_residual", "batch_local_solve", "batch_restrict", "batch_vector", "batch_get_interior",
                 "batch_true_residual_sq"):
        assert callable(getattr(schwz.Subdomain, name))
    assert callable(schwz.SolverRAS.solve_many) and callable(schwz.Csr.spmm) and callable(schwz.BatchCg.solve)


def test_capi_refuses_other_widths_null_arguments_and_a_subdomain_without_a_block_state(schwz):
    """k other than 2, 4, 8, null arguments, a subdomain that was never uploaded: SCHWZ_ERR_INVALID, checked before
    any HIP call (this test runs without a GPU); a preconditioner the block CG does not have: NOT_IMPLEMENTED."""
    lib, c = schwz.capi.lib, schwz.capi
    one, out, iters = np.ones(64 * 8), (ctypes.c_double * 8)(*([7.0] * 8)), (ctypes.c_int * 8)()
    h = ctypes.c_void_p()
    for k in (0, 1, 3, 5, 6, 7, 16, -4):
        assert lib.schwz_csr_spmm(None, k, 1.0, c.ptr(one), 0.0, c.ptr(one), None) == c.ERR_INVALID
        assert b"2, 4 or 8" in lib.schwz_last_error()
        assert lib.schwz_bcg_create(None, 0, k, ctypes.byref(h)) == c.ERR_INVALID and not h.value
        assert lib.schwz_ras_batch_begin(None, k) == c.ERR_INVALID
        assert b"2, 4 or 8" in lib.schwz_last_error()
    assert lib.schwz_csr_spmm(None, 4, 1.0, c.ptr(one), 0.0, c.ptr(one), None) == c.ERR_INVALID
    assert lib.schwz_bcg_create(None, 0, 4, None) == c.ERR_INVALID
    assert lib.schwz_bcg_create(None, 0, 4, ctypes.byref(h)) == c.ERR_INVALID
    assert lib.schwz_bcg_create(None, 9, 4, ctypes.byref(h)) == c.ERR_INVALID
    for precond in (c.PRECOND_BLOCK_JACOBI, c.PRECOND_ILU, c.PRECOND_ISAI):
        assert lib.schwz_bcg_create(None, precond, 4, ctypes.byref(h)) == c.ERR_NOT_IMPLEMENTED
    assert lib.schwz_bcg_solve(None, c.ptr(one), c.ptr(one), 0.0, 1, 0, None, None, None) == c.ERR_INVALID
    assert lib.schwz_bcg_last_stats(None, iters, out) == c.ERR_INVALID
    assert lib.schwz_bcg_residual(None, c.ptr(one), c.ptr(one), None, out, None) == c.ERR_INVALID
    p = schwz.Problem.laplacian(2, 8)
    sd = schwz.Subdomain(p, 1, 0, 2, schwz.partition_regular(64, 1))
    ptr, n = ctypes.c_void_p(), ctypes.c_int64(0)
    for s in (None, sd.h):
        assert lib.schwz_ras_batch_begin(s, 4) == c.ERR_INVALID
        assert lib.schwz_ras_batch_rhs_set(s, c.ptr(one), None) == c.ERR_INVALID
        assert lib.schwz_ras_batch_pack(s, c.ptr(one), None) == c.ERR_INVALID
        assert lib.schwz_ras_batch_unpack(s, c.ptr(one), None) == c.ERR_INVALID
        assert lib.schwz_ras_batch_update_boundary(s, None) == c.ERR_INVALID
        assert lib.schwz_ras_batch_local_residual(s, out, None) == c.ERR_INVALID
        assert lib.schwz_ras_batch_local_solve(s, 0, None, None) == c.ERR_INVALID
        assert lib.schwz_ras_batch_restrict(s, 0, None) == c.ERR_INVALID
        assert lib.schwz_ras_batch_vector(s, 0, ctypes.byref(ptr), ctypes.byref(n)) == c.ERR_INVALID
        assert lib.schwz_ras_batch_get_interior(s, c.ptr(one), None) == c.ERR_INVALID
        assert lib.schwz_ras_batch_true_residual_sq(s, out, None) == c.ERR_INVALID
        assert b"not on the device" in lib.schwz_last_error()
    assert lib.schwz_ras_batch_end(None) == c.ERR_INVALID and lib.schwz_ras_batch_end(sd.h) == c.OK
    assert list(out) == [7.0] * 8  # a refused call writes nothing
    for call in (lambda: sd.batch_begin(4), sd.batch_update_boundary, sd.batch_local_residual, sd.batch_local_solve,
                 sd.batch_restrict, lambda: sd.batch_vector(0), sd.batch_get_interior, sd.batch_true_residual_sq):
        with pytest.raises(schwz.SchwzError) as e:
            call()
        assert e.value.code == c.ERR_INVALID
