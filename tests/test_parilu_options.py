"""The ParILU options (Metadata.par_ilu_sweeps / trisolve_sweeps, schwz_solver_options): defaults, the ABI
struct layout, and the combinations the host refuses before any device call."""
import ctypes

import pytest


def test_metadata_fields_default_to_zero(schwz):
    m = schwz.Metadata()
    assert m.par_ilu_sweeps == 0 and m.trisolve_sweeps == 0


def test_solver_options_end_with_the_two_fields(schwz):
    names = [f[0] for f in schwz.capi.SolverOptions._fields_]
    assert names[-2:] == ["par_ilu_sweeps", "trisolve_sweeps"]
    assert all(f[1] is ctypes.c_int32 for f in schwz.capi.SolverOptions._fields_[-2:])
    # a zero-initialised struct means today's behaviour: the fields are there and zero
    opt = schwz.capi.SolverOptions()
    assert opt.par_ilu_sweeps == 0 and opt.trisolve_sweeps == 0


def _codes(schwz, settings_kw=None, **metadata_kw):
    from schwz_amd import solver as sv
    s = schwz.Settings(**(settings_kw or {}))
    m = schwz.Metadata(**metadata_kw)
    return sv._factor_solver_code(s, m), sv._precond_code(m)


def test_accepted_combinations(schwz):
    c = schwz.capi
    assert _codes(schwz, local_precond="ilu", par_ilu_sweeps=5, trisolve_sweeps=3) == \
        (c.SOLVER_ITERATIVE, c.PRECOND_ILU)
    assert _codes(schwz, local_precond="isai", par_ilu_sweeps=2) == (c.SOLVER_ITERATIVE, c.PRECOND_ISAI)
    assert _codes(schwz, dict(non_symmetric_matrix=True), local_precond="ilu", trisolve_sweeps=1) == \
        (c.SOLVER_ITERATIVE, c.PRECOND_ILU)
    # zeros leave every path as it is
    assert _codes(schwz, local_precond="block-jacobi", precond_max_block_size=1) == \
        (c.SOLVER_ITERATIVE, c.PRECOND_JACOBI)


@pytest.mark.parametrize("settings_kw, metadata_kw", [
    (dict(local_solver="direct-ginkgo"), dict(local_precond="ilu", par_ilu_sweeps=3)),
    (dict(local_solver="direct-cholmod"), dict(local_precond="ilu", trisolve_sweeps=2)),
    (dict(local_solver="direct-ginkgo", factorization="umfpack"), dict(local_precond="null", par_ilu_sweeps=1)),
    (dict(), dict(local_precond="block-jacobi", precond_max_block_size=4, par_ilu_sweeps=3)),
    (dict(), dict(local_precond="block-jacobi", precond_max_block_size=1, trisolve_sweeps=1)),
    (dict(), dict(local_precond="null", par_ilu_sweeps=1)),
    (dict(), dict(local_precond="isai", trisolve_sweeps=2)),
    (dict(), dict(local_precond="isai", par_ilu_sweeps=3, trisolve_sweeps=2)),
])
def test_refused_combinations(schwz, settings_kw, metadata_kw):
    with pytest.raises(schwz.NotImplementedSchwz):
        _codes(schwz, settings_kw, **metadata_kw)


@pytest.mark.parametrize("field", ["par_ilu_sweeps", "trisolve_sweeps"])
def test_negative_counts_are_invalid(schwz, field):
    with pytest.raises(schwz.SchwzError) as e:
        _codes(schwz, local_precond="ilu", **{field: -1})
    assert e.value.code == schwz.capi.ERR_INVALID
    assert not isinstance(e.value, schwz.NotImplementedSchwz)


def test_capi_refuses_before_touching_the_device(schwz):
    """schwz_pcg_create_ilu / schwz_gmres_create_ex check the options before they look at the matrix
    (no GPU needed): NOT_IMPLEMENTED for a wrong preconditioner, INVALID for negative counts."""
    lib, c = schwz.capi.lib, schwz.capi
    h = ctypes.c_void_p()
    assert lib.schwz_pcg_create_ilu(None, c.PRECOND_JACOBI, 2, 0, ctypes.byref(h)) == c.ERR_NOT_IMPLEMENTED
    assert lib.schwz_pcg_create_ilu(None, c.PRECOND_ISAI, 0, 2, ctypes.byref(h)) == c.ERR_NOT_IMPLEMENTED
    assert lib.schwz_pcg_create_ilu(None, c.PRECOND_ILU, -1, 0, ctypes.byref(h)) == c.ERR_INVALID
    assert lib.schwz_gmres_create_ex(None, c.PRECOND_NONE, 1, 10, 0, 3, ctypes.byref(h)) == c.ERR_NOT_IMPLEMENTED
    assert lib.schwz_gmres_create_ex(None, c.PRECOND_ILU, 1, 10, 0, -2, ctypes.byref(h)) == c.ERR_INVALID
    assert not h.value


def test_trs_create_sweeps_checks_its_arguments(schwz):
    """schwz_trs_create_sweeps validates the factors on the host before any upload."""
    import numpy as np
    lrp = np.array([0, 1, 3], np.int32)
    lcol = np.array([0, 0, 1], np.int32)
    lval = np.array([1.0, 0.5, 1.0])
    urp = np.array([0, 2, 3], np.int32)
    ucol = np.array([0, 1, 1], np.int32)
    uval = np.array([2.0, 1.0, 3.0])
    with pytest.raises(schwz.SchwzError):
        schwz.TrsSweeps(lrp, lcol, lval, urp, ucol, uval, 0)
    with pytest.raises(schwz.SchwzError):  # U diagonal not first
        schwz.TrsSweeps(lrp, lcol, lval, urp, np.array([1, 0, 1], np.int32), uval, 2)
    with pytest.raises(schwz.SchwzError):  # zero diagonal
        schwz.TrsSweeps(lrp, lcol, lval, urp, ucol, np.array([0.0, 1.0, 3.0]), 2)
