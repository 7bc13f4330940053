"""The two-level preconditioner of the outer FGMRES: what of it can be checked without a GPU -- the Metadata field
outer_preconditioner, its refusals (raised before the backend or a subdomain is touched), the ABI surface of
schwz_ras_aggregate_sums and its argument checks.  Pattern: tests/test_outer_options.py."""
import os
import re

import numpy as np
import pytest

from test_outer_options import N, NoBackend, NoSubdomain, REFUSED, _invalid, _solver  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGGREGATES = dict(coarse_space="aggregates", coarse_aggregates=4)


def test_field_default(schwz):
    assert schwz.Metadata().outer_preconditioner == "ras"
    from schwz_amd import outer
    assert outer.OUTER_PRECONDITIONERS == ("ras", "two-level")


def test_two_level_with_aggregates_wants_the_loop(schwz):
    """True without a touch of the backend or of a subdomain; with "richardson" the field has no effect."""
    from schwz_amd import outer
    solver = _solver(schwz, outer_iteration="fgmres", outer_preconditioner="two-level", **AGGREGATES)
    assert isinstance(solver.backend, NoBackend) and isinstance(solver.subdomains[0], NoSubdomain)
    assert outer.wants_fgmres(solver.settings, solver.metadata, solver.comm) is True
    for coarse in (AGGREGATES, {}):
        solver = _solver(schwz, outer_iteration="richardson", outer_preconditioner="two-level", **coarse)
        assert outer.wants_fgmres(solver.settings, solver.metadata, solver.comm) is False


@pytest.mark.parametrize("name", ["two_level", "Two-Level", "", "additive", "coarse", None, 2])
@pytest.mark.parametrize("outer_iteration", ["richardson", "fgmres"])
def test_unknown_preconditioners_are_invalid(schwz, outer_iteration, name):
    for set_up in (True, False):
        solver = _solver(schwz, set_up=set_up, outer_iteration=outer_iteration, outer_preconditioner=name)
        assert "outer_preconditioner" in _invalid(schwz, solver.run)
        assert "outer_preconditioner" in _invalid(schwz, solver.initialize)


def test_two_level_without_a_coarse_space_is_invalid(schwz):
    for set_up in (True, False):
        solver = _solver(schwz, set_up=set_up, outer_iteration="fgmres", outer_preconditioner="two-level")
        for call in (solver.run, solver.initialize):
            msg = _invalid(schwz, call)
            assert "two-level" in msg and "coarse_space" in msg


def test_the_default_preconditioner_still_refuses_a_coarse_space(schwz):
    """... and says where to go."""
    solver = _solver(schwz, outer_iteration="fgmres", **AGGREGATES)
    for call in (solver.run, solver.initialize):
        with pytest.raises(schwz.NotImplementedSchwz) as e:
            call()
        assert e.value.code == schwz.capi.ERR_NOT_IMPLEMENTED
        assert "fgmres" in str(e.value) and "outer_preconditioner" in str(e.value) and "two-level" in str(e.value)


@pytest.mark.parametrize("name", sorted(set(REFUSED) - {"coarse space"}))
def test_the_other_refusals_stay_with_two_level(schwz, name):
    """One-sided and overlapped exchange, fp32 halos, the two-stage criterion, several rank processes."""
    config = {k: (dict(v) if isinstance(v, dict) else v) for k, v in REFUSED[name].items()}
    if "onesided" in name:
        # (the coarse space itself refuses the one-sided loops, with NotImplemented too, before the outer check runs)
        expect = ("fgmres", "coarse_space")
    else:
        expect = ("fgmres",)
    for set_up in (True, False):
        solver = _solver(schwz, set_up=set_up, outer_iteration="fgmres", outer_preconditioner="two-level", **AGGREGATES,
                         **config)
        with pytest.raises(schwz.NotImplementedSchwz) as e:
            solver.run()
        assert e.value.code == schwz.capi.ERR_NOT_IMPLEMENTED and "fgmres" in str(e.value)
        with pytest.raises(schwz.NotImplementedSchwz) as e:
            solver.initialize()
        assert e.value.code == schwz.capi.ERR_NOT_IMPLEMENTED and any(w in str(e.value) for w in expect)


def test_new_symbol_is_exported_declared_and_listed(schwz):
    header = open(os.path.join(ROOT, "include", "schwz_hip.h")).read()
    name = "schwz_ras_aggregate_sums"
    assert name in schwz.capi.SYMBOLS
    assert getattr(schwz.capi.lib, name) is not None
    assert re.search(r"\bint\s+%s\(schwz_subdomain \*sd, schwz_coarse \*c, const double \*d_vec, schwz_stream stream\);"
                     % name, header)
    assert len(re.findall(r"\b%s\(" % name, header)) == 1
    assert callable(schwz.Subdomain.aggregate_sums)
    # it matches none of the prefixes whose symbol sets other option tests pin
    for prefix in ("schwz_ras_coarse", "schwz_coarse", "schwz_dense", "schwz_ras_rhs", "schwz_ras_restart", "schwz_outer_",
                   "schwz_ras_apply_interior", "schwz_csr_spmm", "schwz_bcg_", "schwz_ras_batch_", "schwz_cheb",
                   "schwz_ras_cheb"):
        assert not name.startswith(prefix)
    assert "which" in header and re.search(r"\* 3 = one schwz_ras_aggregate_sums", header)


def test_capi_refuses_null_and_mismatched_arguments(schwz):
    """SCHWZ_ERR_INVALID before any HIP call (this test runs without a GPU), and a refused call writes nothing."""
    lib, c = schwz.capi.lib, schwz.capi
    vec = np.full(64, 3.0)
    sd = schwz.Subdomain(schwz.Problem.laplacian(2, 8), 1, 0, 2, schwz.partition_regular(64, 1))
    fake = c.ptr(np.zeros(8))  # (never dereferenced: every call below is refused on its other arguments first)
    assert lib.schwz_ras_aggregate_sums(None, fake, c.ptr(vec), None) == c.ERR_INVALID
    assert b"null argument" in lib.schwz_last_error()
    assert lib.schwz_ras_aggregate_sums(sd.h, None, c.ptr(vec), None) == c.ERR_INVALID
    assert b"null argument" in lib.schwz_last_error()
    assert lib.schwz_ras_aggregate_sums(None, None, None, None) == c.ERR_INVALID
    # a subdomain that is not on the device has no aggregates
    assert lib.schwz_ras_aggregate_sums(sd.h, fake, None, None) == c.ERR_INVALID
    assert b"null argument" in lib.schwz_last_error()
    assert lib.schwz_ras_aggregate_sums(sd.h, fake, c.ptr(vec), None) == c.ERR_INVALID
    assert b"no aggregates" in lib.schwz_last_error()
    with pytest.raises(schwz.SchwzError) as e:
        sd.aggregate_sums(None, 0)
    assert e.value.code == c.ERR_INVALID
    assert lib.schwz_ras_algorithmic_bytes(None, 3) == 0 and sd.algorithmic_bytes(3) == 0
    assert list(vec) == [3.0] * 64
