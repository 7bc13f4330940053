"""The mixed-precision local solve (Metadata.local_solver_precision, schwz_pcg_f32_create): the default, the
combinations the host accepts and refuses before any device call, and the argument checks of the C ABI that need
no GPU."""
import ctypes

import pytest


def test_metadata_field_defaults_to_double(schwz):
    assert schwz.Metadata().local_solver_precision == "double"


def _code(schwz, settings_kw=None, **metadata_kw):
    from schwz_amd import solver as sv
    return sv._precision_code(schwz.Settings(**(settings_kw or {})), schwz.Metadata(**metadata_kw))


def test_accepted_combinations(schwz):
    c = schwz.capi
    assert _code(schwz) == c.PRECISION_F64
    assert _code(schwz, local_solver_precision="double", local_precond="ilu") == c.PRECISION_F64
    assert _code(schwz, dict(local_solver="direct-ginkgo"), local_solver_precision="double") == c.PRECISION_F64
    assert _code(schwz, local_solver_precision="single") == c.PRECISION_F32
    assert _code(schwz, local_solver_precision="single", local_precond="null") == c.PRECISION_F32
    assert _code(schwz, local_solver_precision="single", local_precond="block-jacobi",
                 precond_max_block_size=1) == c.PRECISION_F32


@pytest.mark.parametrize("settings_kw, metadata_kw", [
    (dict(local_solver="direct-ginkgo"), dict()),
    (dict(local_solver="direct-cholmod"), dict()),
    (dict(local_solver="direct-ginkgo", factorization="umfpack"), dict()),
    (dict(non_symmetric_matrix=True), dict()),
    (dict(non_symmetric_matrix=True), dict(local_precond="block-jacobi", precond_max_block_size=1)),
    (dict(), dict(local_precond="block-jacobi", precond_max_block_size=4)),
    (dict(), dict(local_precond="block-jacobi")),   # the default block size is 16
    (dict(), dict(local_precond="ilu")),
    (dict(), dict(local_precond="isai")),
])
def test_refused_combinations(schwz, settings_kw, metadata_kw):
    with pytest.raises(schwz.NotImplementedSchwz):
        _code(schwz, settings_kw, local_solver_precision="single", **metadata_kw)


@pytest.mark.parametrize("name", ["half", "Single", "", None, 1])
def test_unknown_precision_is_invalid(schwz, name):
    with pytest.raises(schwz.SchwzError) as e:
        _code(schwz, local_solver_precision=name)
    assert e.value.code == schwz.capi.ERR_INVALID
    assert not isinstance(e.value, schwz.NotImplementedSchwz)


def test_initialize_refuses_before_any_device_call(schwz):
    """The validator runs at the top of initialize(): no matrix is set up, no subdomain created."""
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(4, 4, 4))
    m = schwz.Metadata(num_subdomains=1, local_solver_precision="single", local_precond="ilu")

    class NoBackend:
        def __getattr__(self, name):
            raise AssertionError("the backend was touched: %s" % name)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(1), backend=NoBackend(), quiet=True)
    with pytest.raises(schwz.NotImplementedSchwz):
        solver.initialize()


def test_capi_refuses_before_touching_the_matrix(schwz):
    """schwz_pcg_f32_create checks the preconditioner code and the output pointer before it looks at the matrix."""
    lib, c = schwz.capi.lib, schwz.capi
    h = ctypes.c_void_p()
    assert lib.schwz_pcg_f32_create(None, c.PRECOND_ILU, ctypes.byref(h)) == c.ERR_NOT_IMPLEMENTED
    assert lib.schwz_pcg_f32_create(None, c.PRECOND_ISAI, ctypes.byref(h)) == c.ERR_NOT_IMPLEMENTED
    assert lib.schwz_pcg_f32_create(None, c.PRECOND_BLOCK_JACOBI, ctypes.byref(h)) == c.ERR_NOT_IMPLEMENTED
    assert lib.schwz_pcg_f32_create(None, 99, ctypes.byref(h)) == c.ERR_INVALID
    assert lib.schwz_pcg_f32_create(None, -1, ctypes.byref(h)) == c.ERR_INVALID
    assert lib.schwz_pcg_f32_create(None, c.PRECOND_JACOBI, None) == c.ERR_INVALID
    # accepted codes get as far as the matrix, which is missing
    assert lib.schwz_pcg_f32_create(None, c.PRECOND_JACOBI, ctypes.byref(h)) == c.ERR_INVALID
    assert not h.value
    assert (c.PRECISION_F64, c.PRECISION_F32) == (0, 1)
    # no subdomain: double
    assert lib.schwz_ras_local_precision(None) == c.PRECISION_F64
    assert lib.schwz_ras_set_local_precision(None, c.PRECISION_F32) == c.ERR_INVALID


def test_solver_options_are_unchanged(schwz):
    """The precision travels through schwz_ras_set_local_precision: the options struct keeps its layout."""
    assert [(n, t) for n, t in schwz.capi.SolverOptions._fields_] == [
        ("local_solver", ctypes.c_int32), ("precond", ctypes.c_int32), ("local_tol", ctypes.c_double),
        ("local_max_iters", ctypes.c_int32), ("natural_factor_ordering", ctypes.c_int32),
        ("spmv_variant", ctypes.c_int32), ("precond_block_size", ctypes.c_int32), ("non_symmetric", ctypes.c_int32),
        ("restart_iter", ctypes.c_int32), ("par_ilu_sweeps", ctypes.c_int32), ("trisolve_sweeps", ctypes.c_int32)]
    assert ctypes.sizeof(schwz.capi.SolverOptions) == 48   # 2 x int32, double, 8 x int32
