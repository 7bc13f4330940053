"""The coarse space of the two-level RAS (Metadata.coarse_space / coarse_aggregates / coarse_aggregate_vector,
schwz_ras_coarse_*, schwz_coarse_*, schwz_dense_inverse): the defaults, what the host accepts and refuses before any
device call, how a caller's aggregate vector is split by owner, and the argument checks of the C ABI that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["schwz_ras_coarse_set_aggregates", "schwz_ras_coarse_rows", "schwz_dense_inverse", "schwz_coarse_create",
               "schwz_coarse_destroy", "schwz_coarse_vector", "schwz_ras_coarse_residual", "schwz_coarse_solve",
               "schwz_ras_coarse_apply"]


def _enabled(schwz, settings_kw=None, onesided=False, **metadata_kw):
    from schwz_amd import solver as sv
    s = schwz.Settings(**(settings_kw or {}))
    s.comm_settings.enable_onesided = onesided
    return sv._coarse_enabled(s, schwz.Metadata(**metadata_kw))


def test_metadata_defaults(schwz):
    m = schwz.Metadata()
    assert (m.coarse_space, m.coarse_aggregates, m.coarse_aggregate_vector) == ("none", 0, None)
    assert _enabled(schwz) is False
    # "none" reads none of the other fields and accepts every loop
    assert _enabled(schwz, onesided=True, coarse_aggregates=-3, coarse_aggregate_vector=[-1]) is False


def test_accepted_combinations(schwz):
    assert _enabled(schwz, coarse_space="aggregates", coarse_aggregates=8) is True
    assert _enabled(schwz, coarse_space="aggregates", coarse_aggregate_vector=np.arange(10)) is True
    assert _enabled(schwz, coarse_space="aggregates", coarse_aggregate_vector=[0, 0, 3, 3], coarse_aggregates=0) is True
    assert _enabled(schwz, dict(overlap=1), coarse_space="aggregates", coarse_aggregates=2, num_subdomains=1) is True
    assert _enabled(schwz, coarse_space="aggregates", coarse_aggregates=512, num_subdomains=8) is True


@pytest.mark.parametrize("name", ["aggregate", "Aggregates", "NONE", "", None, 1, "smoothed"])
def test_unknown_coarse_space_is_invalid(schwz, name):
    with pytest.raises(schwz.SchwzError) as e:
        _enabled(schwz, coarse_space=name, coarse_aggregates=4)
    assert e.value.code == schwz.capi.ERR_INVALID
    assert not isinstance(e.value, schwz.NotImplementedSchwz)


@pytest.mark.parametrize("mkw", [dict(), dict(coarse_aggregates=0), dict(coarse_aggregates=-2),
                                 dict(coarse_aggregates=None)])
def test_aggregates_need_a_count_or_a_vector(schwz, mkw):
    with pytest.raises(schwz.SchwzError) as e:
        _enabled(schwz, coarse_space="aggregates", **mkw)
    assert e.value.code == schwz.capi.ERR_INVALID


@pytest.mark.parametrize("vec", [[0, 1, -1, 2], np.array([[0, 1], [2, 3]]), np.array([0.0, 1.0]), 3])
def test_bad_vectors_are_invalid(schwz, vec):
    with pytest.raises(schwz.SchwzError) as e:
        _enabled(schwz, coarse_space="aggregates", coarse_aggregate_vector=vec)
    assert e.value.code == schwz.capi.ERR_INVALID


def test_vector_of_the_wrong_length_is_invalid(schwz):
    from schwz_amd import solver as sv
    m = schwz.Metadata(coarse_space="aggregates", coarse_aggregate_vector=np.zeros(63, dtype=np.int64))
    with pytest.raises(schwz.SchwzError) as e:
        sv._coarse_vector(m, 64)
    assert e.value.code == schwz.capi.ERR_INVALID and "64 rows" in str(e.value)
    assert sv._coarse_vector(schwz.Metadata(coarse_aggregate_vector=list(range(64))), 64).dtype == np.int64


def test_refusals_that_are_not_implemented(schwz):
    c = schwz.capi
    for kw in (dict(onesided=True, coarse_aggregates=4),
               dict(settings_kw=dict(overlap=1), coarse_aggregates=4, num_subdomains=2),
               dict(coarse_aggregates=513, num_subdomains=8)):  # 4104 aggregates
        with pytest.raises(schwz.NotImplementedSchwz) as e:
            _enabled(schwz, coarse_space="aggregates", **kw)
        assert e.value.code == c.ERR_NOT_IMPLEMENTED
    assert c.COARSE_MAX_DOFS == 4096


def test_the_vector_is_split_by_owner_and_compacted(schwz):
    """Rows of one id in different subdomains become different aggregates; ids are compacted; the ids of subdomain p
    are the range [first[p], first[p + 1]), empty subdomains included."""
    from schwz_amd import solver as sv
    ids, first = sv._split_aggregates(np.array([5, 5, 7, 7, 5, 5, 9, 9]), [0, 3, 8, 8])
    assert list(ids) == [0, 0, 1, 3, 2, 2, 4, 4] and list(first) == [0, 2, 5, 5]
    ids, first = sv._split_aggregates(np.array([40, 2, 2]), [0, 1, 2, 3, 3, 3])
    assert list(ids) == [0, 1, 2] and list(first) == [0, 1, 2, 3, 3, 3]


@pytest.mark.parametrize("mkw,onesided,code", [
    (dict(coarse_space="boxes"), False, "ERR_INVALID"),
    (dict(coarse_space="aggregates"), False, "ERR_INVALID"),
    (dict(coarse_space="aggregates", coarse_aggregate_vector=[0, -1]), False, "ERR_INVALID"),
    (dict(coarse_space="aggregates", coarse_aggregates=4), True, "ERR_NOT_IMPLEMENTED")])
def test_initialize_refuses_before_any_device_call(schwz, mkw, onesided, code):
    """The validator runs at the top of initialize(): no matrix is set up, no subdomain created."""
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=(4, 4, 4))
    s.comm_settings.enable_onesided = onesided
    s.convergence_settings.enable_global_simple_tree = onesided
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
    declared = set(re.findall(r"\b(schwz_(?:ras_coarse|coarse|dense)\w*)\(", header))
    assert declared == set(NEW_SYMBOLS), declared ^ set(NEW_SYMBOLS)


def test_dense_inverse(schwz):
    """LU with partial pivoting: a matrix that needs row exchanges, a random non-symmetric one, and the documented
    refusal of a singular one (the coarse matrix of a pure Neumann problem)."""
    a = np.array([[0.0, 2.0, 1.0], [1.0, 0.0, 0.0], [4.0, 1.0, 1.5]])
    assert np.abs(schwz.dense_inverse(a) @ a - np.eye(3)).max() <= 1e-15
    rng = np.random.default_rng(5)
    a = rng.standard_normal((257, 257)) + 12.0 * np.eye(257)
    assert np.abs(schwz.dense_inverse(a) @ a - np.eye(257)).max() <= 1e-12
    for bad in (np.array([[1.0, -1.0, 0.0], [-1.0, 2.0, -1.0], [0.0, -1.0, 1.0]]), np.zeros((2, 2)),
                np.array([[1.0, 2.0], [float("nan"), 1.0]]), np.array([[2.0, 0.0], [0.0, 0.0]])):
        with pytest.raises(schwz.SchwzError) as e:
            schwz.dense_inverse(bad)
        assert e.value.code == schwz.capi.ERR_INVALID
        assert "singular" in str(e.value) and "Neumann" in str(e.value) and "aggregate" in str(e.value)


def test_capi_refuses_without_touching_a_device(schwz):
    lib, c = schwz.capi.lib, schwz.capi
    h = ctypes.c_void_p()
    one = np.ones(1)
    for nc in (0, -1, 4097):
        assert lib.schwz_coarse_create(nc, c.ptr(one), ctypes.byref(h)) == c.ERR_INVALID and not h.value
    assert lib.schwz_coarse_create(1, None, ctypes.byref(h)) == c.ERR_INVALID
    assert lib.schwz_coarse_create(1, c.ptr(one), None) == c.ERR_INVALID
    lib.schwz_coarse_destroy(None)
    p, n = ctypes.c_void_p(), ctypes.c_int32(0)
    assert lib.schwz_coarse_vector(None, 0, ctypes.byref(p), ctypes.byref(n)) == c.ERR_INVALID
    assert lib.schwz_coarse_solve(None, None) == c.ERR_INVALID
    assert lib.schwz_ras_coarse_residual(None, None, None) == c.ERR_INVALID
    assert lib.schwz_ras_coarse_apply(None, None, None) == c.ERR_INVALID
    assert lib.schwz_ras_coarse_rows(None, None) == c.ERR_INVALID
    assert lib.schwz_ras_coarse_set_aggregates(None, None, 0, 0, 1) == c.ERR_INVALID
    assert lib.schwz_ras_algorithmic_bytes(None, 2) == 0


def test_entry_points_need_a_subdomain_on_the_device(schwz):
    p = schwz.Problem.laplacian(2, 8)
    sd = schwz.Subdomain(p, 1, 0, 2, schwz.partition_regular(64, 1))
    with pytest.raises(schwz.SchwzError) as e:
        sd.coarse_set_aggregates(np.zeros(64, dtype=np.int32), 0, 1, 1)
    assert e.value.code == schwz.capi.ERR_INVALID
    assert sd.algorithmic_bytes(2) == 0
