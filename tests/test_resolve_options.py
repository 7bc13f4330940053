"""One matrix, many right-hand sides: what of SolverRAS.set_rhs / solve and of the schwz_ras_rhs_* / schwz_ras_restart
entry points can be checked without a GPU -- the refusals (all before any device call, all ERR_INVALID and none a
NotImplementedSchwz), the ABI surface and the argument checks of the library."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["schwz_ras_rhs_set", "schwz_ras_rhs_index", "schwz_ras_rhs_gather", "schwz_ras_rhs_aggregate",
               "schwz_ras_rhs_norm_sq", "schwz_ras_rhs_norm_sq_local", "schwz_ras_restart"]
N = 12


class NoBackend:
    """Any use of the backend is a device call made too early."""

    def __getattr__(self, name):
        raise AssertionError("the backend was touched: %s" % name)


class TorchOnlyBackend:
    """What the checks of a tensor may look at: the torch module and the solver's device.  Nothing else."""

    def __init__(self):
        import torch
        self.__dict__["_torch"] = torch
        self.__dict__["device"] = torch.device("cuda", 0)

    def __getattr__(self, name):
        raise AssertionError("the backend was touched: %s" % name)


class NoSubdomain:
    def __getattr__(self, name):
        raise AssertionError("a subdomain was touched: %s" % name)


def _solver(schwz, backend=None, set_up=True):
    m = schwz.Metadata(num_subdomains=1)
    solver = schwz.SolverRAS(schwz.Settings(), m, comm=schwz.InProcessComm(1), backend=backend or NoBackend(), quiet=True)
    if set_up:  # what initialize() leaves, as far as the checks look: a problem, subdomains, the global size
        solver.problem = object()
        solver.subdomains = {0: NoSubdomain()}
        m.global_size = N
    return solver


def _refused(schwz, call):
    with pytest.raises(schwz.SchwzError) as e:
        call()
    assert e.value.code == schwz.capi.ERR_INVALID, e.value
    assert not isinstance(e.value, schwz.NotImplementedSchwz)
    return str(e.value)


@pytest.mark.parametrize("method", ["set_rhs", "solve"])
def test_refused_before_initialize(schwz, method):
    solver = _solver(schwz, set_up=False)
    assert "initialize" in _refused(schwz, lambda: getattr(solver, method)(np.ones(N)))
    assert "initialize" in _refused(schwz, lambda: getattr(solver, method)())


@pytest.mark.parametrize("bad", [
    np.ones(N - 1), np.ones(N + 1), np.ones((N, 1)), np.ones((2, N // 2)), np.float64(1.0),          # length, rank
    np.ones(N, dtype=np.int64), np.ones(N, dtype=bool), np.ones(N, dtype=np.complex128), ["a"] * N,  # not floats
    np.r_[np.ones(N - 1), np.nan], np.r_[np.inf, np.ones(N - 1)], np.r_[np.ones(N - 1), -np.inf],    # not finite
], ids=["short", "long", "column", "matrix", "scalar", "int64", "bool", "complex", "strings", "nan", "inf", "-inf"])
def test_host_arrays_refused(schwz, bad):
    solver = _solver(schwz)
    _refused(schwz, lambda: solver.set_rhs(bad))
    _refused(schwz, lambda: solver.solve(bad))
    assert solver._user_rhs is None and solver._device_rhs is None  # nothing was taken over


@pytest.mark.parametrize("guess", ["", "zeros", "warm", None, 0, "KEEP"])
def test_unknown_initial_guess_refused(schwz, guess):
    solver = _solver(schwz)
    assert "initial_guess" in _refused(schwz, lambda: solver.set_rhs(np.ones(N), initial_guess=guess))
    assert "initial_guess" in _refused(schwz, lambda: solver.set_rhs(None, guess))


def test_tensors_refused(schwz):
    """Another dtype, another shape, another device (a host tensor; the solver lives on cuda:0)."""
    import torch
    solver = _solver(schwz, backend=TorchOnlyBackend())
    for bad in (torch.ones(N, dtype=torch.float32), torch.ones(N, dtype=torch.int64), torch.ones(N, dtype=torch.float16)):
        assert "float64" in _refused(schwz, lambda: solver.set_rhs(bad))
    for bad in (torch.ones(N - 1, dtype=torch.float64), torch.ones((N, 1), dtype=torch.float64),
                torch.ones((), dtype=torch.float64)):
        assert "shape" in _refused(schwz, lambda: solver.set_rhs(bad))
    assert "cpu" in _refused(schwz, lambda: solver.set_rhs(torch.ones(N, dtype=torch.float64)))
    assert solver._user_rhs is None and solver._device_rhs is None


def test_new_symbols_are_exported_declared_and_listed(schwz):
    header = open(os.path.join(ROOT, "include", "schwz_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in schwz.capi.SYMBOLS
        assert getattr(schwz.capi.lib, name) is not None
        assert getattr(schwz.capi.lib, name).argtypes is not None
        assert re.search(r"\bint\s+%s\(" % name, header), name
    declared = set(re.findall(r"\b(schwz_ras_(?:rhs|restart)\w*)\(", header))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)
    for name in ("rhs_set", "rhs_index", "rhs_gather", "rhs_aggregate", "rhs_norm_sq", "rhs_norm_sq_local", "restart"):
        assert callable(getattr(schwz.Subdomain, name))
    assert callable(schwz.SolverRAS.set_rhs) and callable(schwz.SolverRAS.solve)


def test_capi_refuses_null_arguments_and_a_subdomain_that_is_not_on_the_device(schwz):
    """Null arguments and a subdomain that was never uploaded: SCHWZ_ERR_INVALID, checked before any HIP call (this
    test runs without a GPU)."""
    lib, c = schwz.capi.lib, schwz.capi
    one, idx, out = np.ones(64), np.zeros(64, dtype=np.int64), ctypes.c_double(7.0)
    p = schwz.Problem.laplacian(2, 8)
    sd = schwz.Subdomain(p, 1, 0, 2, schwz.partition_regular(64, 1))
    for h in (None, sd.h):
        assert lib.schwz_ras_rhs_set(h, c.ptr(one), 0, None) == c.ERR_INVALID
        assert lib.schwz_ras_rhs_set(h, c.ptr(one), 1, None) == c.ERR_INVALID
        assert lib.schwz_ras_rhs_index(h, c.ptr(idx)) == c.ERR_INVALID
        assert lib.schwz_ras_rhs_index(h, None) == c.ERR_INVALID
        assert lib.schwz_ras_rhs_gather(h, c.ptr(one), 64, None) == c.ERR_INVALID
        assert lib.schwz_ras_rhs_aggregate(h, None) == c.ERR_INVALID
        assert lib.schwz_ras_rhs_norm_sq(h, ctypes.byref(out), None) == c.ERR_INVALID
        assert lib.schwz_ras_rhs_norm_sq_local(h, ctypes.byref(out), None) == c.ERR_INVALID
        assert lib.schwz_ras_restart(h, 0, None) == c.ERR_INVALID
        assert lib.schwz_ras_restart(h, 1, None) == c.ERR_INVALID
        assert b"not on the device" in lib.schwz_last_error()
    assert out.value == 7.0  # a refused call writes nothing
    for call in (lambda: sd.rhs_set(one), lambda: sd.rhs_index(None), lambda: sd.rhs_index(idx),
                 lambda: sd.rhs_gather(0, 64), sd.rhs_aggregate, sd.rhs_norm_sq, sd.rhs_norm_sq_local, sd.restart):
        _refused(schwz, call)
