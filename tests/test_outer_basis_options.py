"""The fp32-compressed basis of the outer FGMRES: what of it can be checked without a GPU -- the Metadata field
outer_basis, that every refusal of the loop still fires with it, the ABI surface of the four new entry points and
their argument checks.  Pattern: tests/test_outer_coarse_options.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_outer_options import N, NoBackend, NoSubdomain, REFUSED, _invalid, _solver  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["schwz_outer_create_basis", "schwz_outer_basis_read", "schwz_outer_basis_write", "schwz_outer_residual"]
AGGREGATES = dict(coarse_space="aggregates", coarse_aggregates=4)


def test_field_default(schwz):
    assert schwz.Metadata().outer_basis == "double"
    from schwz_amd import outer
    assert outer.OUTER_BASES == ("double", "single")
    assert schwz.capi.OUTER_BASIS == {"double": 0, "single": 1}


@pytest.mark.parametrize("name", ["float", "fp32", "", "Single", "SINGLE", "Double", None, 1, 0, np.float32, b"single"])
@pytest.mark.parametrize("outer_iteration", ["richardson", "fgmres"])
def test_unknown_bases_are_invalid(schwz, outer_iteration, name):
    for set_up in (True, False):
        solver = _solver(schwz, set_up=set_up, outer_iteration=outer_iteration, outer_basis=name)
        assert "outer_basis" in _invalid(schwz, solver.run)
        assert "outer_basis" in _invalid(schwz, solver.initialize)


def test_single_under_richardson_changes_nothing(schwz):
    from schwz_amd import outer
    for config in ({}, AGGREGATES, REFUSED["fp32 halos"], REFUSED["two-stage"]):
        solver = _solver(schwz, outer_iteration="richardson", outer_basis="single", **config)
        assert outer.wants_fgmres(solver.settings, solver.metadata, solver.comm) is False


@pytest.mark.parametrize("config", [
    dict(), dict(outer_restart=5), dict(outer_restart=128), dict(outer_preconditioner="two-level", **AGGREGATES),
    dict(settings=dict(local_solver="direct-cholmod")),
    dict(settings=dict(local_solver="direct-ginkgo", factorization="umfpack", non_symmetric_matrix=True)),
    dict(settings=dict(non_symmetric_matrix=True), gmres_basis="single"), dict(local_solver_precision="single"),
], ids=["default", "restart 5", "restart 128", "two-level", "cholmod", "umfpack", "fp32 local basis", "fp32 cg"])
def test_single_under_fgmres_wants_the_loop(schwz, config):
    """True without a touch of the backend or of a subdomain."""
    from schwz_amd import outer
    for basis in ("single", "double"):
        solver = _solver(schwz, outer_iteration="fgmres", outer_basis=basis, **config)
        assert isinstance(solver.backend, NoBackend) and isinstance(solver.subdomains[0], NoSubdomain)
        assert outer.wants_fgmres(solver.settings, solver.metadata, solver.comm) is True


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_every_refusal_still_fires_with_single(schwz, name):
    for set_up in (True, False):
        solver = _solver(schwz, set_up=set_up, outer_iteration="fgmres", outer_basis="single", **REFUSED[name])
        for call in (solver.run, solver.initialize):
            with pytest.raises(schwz.NotImplementedSchwz) as e:
                call()
            assert e.value.code == schwz.capi.ERR_NOT_IMPLEMENTED and "fgmres" in str(e.value)


def test_the_other_fields_are_still_checked_with_single(schwz):
    solver = _solver(schwz, outer_iteration="fgmres", outer_basis="single", outer_restart=129)
    assert "outer_restart" in _invalid(schwz, solver.run)
    solver = _solver(schwz, outer_iteration="fgmres", outer_basis="single", outer_preconditioner="additive")
    assert "outer_preconditioner" in _invalid(schwz, solver.run)
    solver = _solver(schwz, outer_iteration="fgmres", outer_basis="single", outer_preconditioner="two-level")
    assert "coarse_space" in _invalid(schwz, solver.run)
    solver = _solver(schwz, set_up=False, outer_iteration="fgmres", outer_basis="single")
    assert "initialize" in _invalid(schwz, solver.run)


def test_solve_many_ignores_the_field(schwz):
    solver = _solver(schwz, outer_iteration="fgmres", outer_basis="single", local_precond="block-jacobi",
                     precond_max_block_size=1)
    assert "shape" in _invalid(schwz, lambda: solver.solve_many(np.ones(N)))


def test_new_symbols_are_exported_declared_and_listed(schwz):
    header = open(os.path.join(ROOT, "include", "schwz_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in schwz.capi.SYMBOLS
        assert getattr(schwz.capi.lib, name) is not None
        assert getattr(schwz.capi.lib, name).argtypes is not None
        assert len(re.findall(r"\bint\s+%s\s*\(" % name, header)) == 1, name
    assert re.search(r"enum schwz_outer_basis \{ SCHWZ_OUTER_BASIS_F64 = 0, SCHWZ_OUTER_BASIS_F32 = 1 \};", header)
    for method in ("basis_read", "basis_write", "residual"):
        assert callable(getattr(schwz.Outer, method))
    assert "12 n (j + 1) + 52 n" in header and "2^-24" in header


def test_capi_refuses_null_and_out_of_range_arguments(schwz):
    """SCHWZ_ERR_INVALID before any HIP call (this test runs without a GPU), and a refused call writes nothing."""
    lib, c = schwz.capi.lib, schwz.capi
    one, out = np.ones(64), np.full(8, 7.0)
    h = ctypes.c_void_p()
    assert lib.schwz_outer_create_basis(16, 5, 1, None) == c.ERR_INVALID
    for n, restart, basis in ((-1, 5, 1), (16, 0, 1), (16, 129, 1), (16, 5, 2), (16, 5, -1)):
        assert lib.schwz_outer_create_basis(n, restart, basis, ctypes.byref(h)) == c.ERR_INVALID and not h.value
    assert b"basis" in lib.schwz_last_error()
    assert lib.schwz_outer_basis_read(None, 0, 0, 1, c.ptr(one), None) == c.ERR_INVALID
    assert lib.schwz_outer_basis_write(None, 0, 0, 1, c.ptr(one), None) == c.ERR_INVALID
    assert lib.schwz_outer_residual(None, c.ptr(one), c.ptr(out), None) == c.ERR_INVALID
    assert list(out) == [7.0] * 8 and list(one) == [1.0] * 64
