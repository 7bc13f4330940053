"""CPU tests of the product's host code (libschwz_hip.so, no GPU calls):
the ABI surface, and bit-exact parity of problem generation / partitioning /
subdomain index sets / comm lists / LL^T structure with the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")


def test_abi_exports_every_declared_symbol(schwz):
    header = open(os.path.join(ROOT, "include", "schwz_hip.h")).read()
    declared = set(re.findall(r"\b(schwz_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(schwz.capi.LIB_PATH)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert declared == set(schwz.capi.SYMBOLS)


def test_version_and_device_count(schwz):
    assert b"gfx950" in schwz.capi.lib.schwz_version()
    assert schwz.capi.device_count() >= 0


def test_product_fails_loudly_without_gpu(schwz):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    s = schwz.Settings()
    m = schwz.Metadata(oned_laplacian_size=8, num_subdomains=2)
    with pytest.raises(schwz.SchwzError):
        schwz.SolverRAS(s, m).initialize()
    p = schwz.Problem.laplacian(2, 8)
    sd = schwz.Subdomain(p, 1, 0, 2, schwz.partition_regular(64, 1))
    with pytest.raises(schwz.SchwzError):
        sd.to_device(np.ones(sd.local_size_x))


def test_cpu_executors_are_refused(schwz):
    for ex in ("reference", "omp"):
        with pytest.raises(schwz.NotImplementedSchwz):
            schwz.SolverRAS(schwz.Settings(executor_string=ex), schwz.Metadata())


@pytest.mark.parametrize("dim,shape", [(2, (13,)), (3, (5, 4, 3)), (3, (7, 7, 7))])
def test_problem_rows_match_oracle(schwz, oracle, dim, shape):
    if dim == 2:
        p = schwz.Problem.laplacian(2, shape[0])
        o = oracle.laplacian2d(shape[0])
    else:
        p = schwz.Problem.laplacian(3, *shape)
        o = oracle.laplacian3d(*shape)
    rp, col, val = p.to_csr()
    assert np.array_equal(rp, o[0]) and np.array_equal(col, o[1]) and np.array_equal(val, o[2])
    assert p.nnz == o[0][-1]


def test_matrix_market_reader(schwz, tmp_path):
    g = np.load(os.path.join(G, "ani3_crop.npz"))
    n = len(g["rp"]) - 1
    path = tmp_path / "m.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n% comment\n")
        f.write("%d %d %d\n" % (n, n, g["rp"][-1]))
        rows = np.repeat(np.arange(n), np.diff(g["rp"]))
        # shuffled order: the reader must sort by column (initialization.cpp:212)
        order = np.random.default_rng(0).permutation(len(rows))
        for k in order:
            f.write("%d %d %.17g\n" % (rows[k] + 1, g["col"][k] + 1, g["val"][k]))
    p = schwz.Problem.from_matrix_market(str(path))
    rp, col, val = p.to_csr()
    assert np.array_equal(rp, g["rp"]) and np.array_equal(col, g["col"]) and np.array_equal(val, g["val"])
    with pytest.raises(schwz.SchwzError):
        schwz.Problem.from_matrix_market(str(tmp_path / "missing.mtx"))


def _compare_subdomains(schwz, oracle, prob, csr, P, overlap, fr):
    orp, ocol, oval = csr
    sds, osds = [], []
    for me in range(P):
        sd = schwz.Subdomain(prob, P, me, overlap, fr)
        osd = oracle.Subdomain(orp, ocol, oval, P, me, overlap, fr.astype(np.int32))
        for a, b in zip(sd.local_matrix(), osd.local_matrix()):
            assert np.array_equal(a, b)
        for a, b in zip(sd.interface_matrix(), osd.interface_matrix()):
            assert np.array_equal(a, b)
        assert np.array_equal(sd.local_to_global, osd.local_to_global)
        g1, g2 = sd.get_lists(), osd.get_lists()
        assert [r for r, _ in g1] == [r for r, _ in g2]
        for (_, a), (_, b) in zip(g1, g2):
            assert np.array_equal(a, b)
        assert (sd.local_size, sd.local_size_x, sd.overlap_size, sd.halo_size, sd.nnz_local,
                sd.nnz_interface, sd.num_recv) == \
               (osd.local_size, osd.local_size_x, osd.overlap_size, osd.halo_size, osd.nnz_local,
                osd.nnz_interface, osd.num_recv)
        sds.append(sd)
        osds.append(osd)
    oracle.connect(osds)
    puts = schwz.InProcessComm(P).handshake({me: sd.get_lists() for me, sd in enumerate(sds)})
    for me, sd in enumerate(sds):
        for q, ids in puts[me]:
            sd.add_put_list(q, ids)
        p1, p2 = sd.put_lists(), osds[me].put_lists()
        assert [r for r, _ in p1] == [r for r, _ in p2]
        for (_, a), (_, b) in zip(p1, p2):
            assert np.array_equal(a, b)
        assert sd.num_send == osds[me].num_send
        assert sd.send_offsets()[-1] == sd.num_send and sd.recv_offsets()[-1] == sd.num_recv


@pytest.mark.parametrize("P", [1, 2, 3, 8])
@pytest.mark.parametrize("overlap", [1, 2, 3, 5])
def test_subdomain_index_sets_2d(schwz, oracle, P, overlap):
    n = 12
    prob = schwz.Problem.laplacian(2, n)
    _compare_subdomains(schwz, oracle, prob, oracle.laplacian2d(n), P, overlap,
                        schwz.partition_regular(n * n, P))


@pytest.mark.parametrize("P", [2, 4, 7])
def test_subdomain_index_sets_3d_ragged_slabs(schwz, oracle, P):
    shape = (5, 4, 9)  # N=180: slabs cut through planes for P=7
    prob = schwz.Problem.laplacian(3, *shape)
    _compare_subdomains(schwz, oracle, prob, oracle.laplacian3d(*shape), P, 2,
                        schwz.partition_regular(180, P))


def test_subdomain_index_sets_general_matrix(schwz, oracle):
    g = np.load(os.path.join(G, "ani3_crop.npz"))
    prob = schwz.Problem.from_csr(g["rp"], g["col"], g["val"])
    N = prob.N
    _compare_subdomains(schwz, oracle, prob, (g["rp"], g["col"], g["val"]), 8, 2,
                        schwz.partition_regular(N, 8))
    _compare_subdomains(schwz, oracle, prob, (g["rp"], g["col"], g["val"]), 4, 4,
                        schwz.partition_regular(N, 4))


def test_partition_vector_permutation_matches_oracle(schwz, oracle):
    n, P = 8, 4
    part = schwz.partition_regular2d(n, P)
    assert np.array_equal(part, oracle.partition_regular2d(n, P))
    prob = schwz.Problem.laplacian(2, n)
    pprob, perm, fr = prob.permute(part, P)
    operm, oiperm, ofr, orp, ocol, oval = oracle.apply_partition(*oracle.laplacian2d(n), part, P)
    assert np.array_equal(perm, operm) and np.array_equal(fr, ofr)
    rp, col, val = pprob.to_csr()
    # the product keeps permuted rows column-sorted; same entries per row
    for i in range(n * n):
        a = sorted(zip(col[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]))
        b = sorted(zip(ocol[orp[i]:orp[i + 1]], oval[orp[i]:orp[i + 1]]))
        assert a == b
    with pytest.raises(schwz.SchwzError):
        schwz.partition_regular2d(8, 3)


def test_graph_partition_is_balanced_and_connected_enough(schwz):
    g = np.load(os.path.join(G, "ani4_crop.npz"))
    prob = schwz.Problem.from_csr(g["rp"], g["col"], g["val"])
    part = prob.partition_graph(8)
    counts = np.bincount(part, minlength=8)
    assert counts.sum() == prob.N and counts.min() >= prob.N // 8 - 2 and counts.max() <= prob.N // 8 + 2
    # edge cut far below a random assignment
    rows = np.repeat(np.arange(prob.N), np.diff(g["rp"]))
    cut = np.count_nonzero(part[rows] != part[g["col"]])
    assert cut < 0.15 * len(rows)


def test_graph_partition_multilevel_quality(schwz, oracle):
    """The multilevel recursive bisection (heavy-edge coarsening, greedy growing, FM refinement at every level;
    what PartitionMetis would get from METIS, include/partition_tools.hpp:110-202).  Cuts are counted as
    UNDIRECTED edges (an off-diagonal entry pair counts once): on a 24^3 grid in 8 parts the 2 x 2 x 2 block
    partition cuts 3 * 24^2 = 1728 edges; the single-level bisection of rounds 1-2 cut 2170 (1.26 x), the
    multilevel scheme must stay within 1.05 x at EXACT balance.  Also odd part counts and a 2-D grid."""
    def cut_and_sizes(rp, col, P):
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        prob = schwz.Problem.from_csr(rp, col, np.ones(len(col)))
        part = prob.partition_graph(P)
        return np.count_nonzero(part[rows] != part[col]) // 2, np.bincount(part, minlength=P)
    rp, col, _ = oracle.laplacian3d(24, 24, 24)
    cut, sizes = cut_and_sizes(rp, col, 8)
    assert (sizes == 1728).all()
    assert cut <= 1.05 * 1728, cut
    cut, sizes = cut_and_sizes(rp, col, 3)
    assert sizes.sum() == 24 ** 3 and sizes.max() - sizes.min() <= 1
    assert cut <= 1.25 * 2 * 24 * 24, cut     # two planes would cut 1152
    rp, col, _ = oracle.laplacian2d(60)
    cut, sizes = cut_and_sizes(rp, col, 4)
    assert (sizes == 900).all() and cut <= 1.1 * 120, cut
    # the same call twice gives the same partition (no random numbers)
    prob = schwz.Problem.from_csr(rp, col, np.ones(len(col)))
    assert np.array_equal(prob.partition_graph(5), prob.partition_graph(5))


@pytest.mark.parametrize("natural", [True, False])
def test_cholesky_matches_oracle_structure_and_values(schwz, oracle, natural):
    g = np.load(os.path.join(G, "ani3_crop.npz"))
    f = schwz.cholesky(g["rp"], g["col"], g["val"], natural)
    fo = oracle.cholesky(g["rp"], g["col"], g["val"], natural)
    for k in ("perm", "l_rp", "l_col", "u_rp", "u_col"):
        assert np.array_equal(f[k], fo[k]), k
    assert np.abs(f["l_val"] - fo["l_val"]).max() <= 1e-12 * np.abs(fo["l_val"]).max()
    # identity A(perm,perm) = L L^T
    import scipy.sparse as sp
    n = len(g["rp"]) - 1
    A = sp.csr_matrix((g["val"], g["col"], g["rp"]), shape=(n, n))
    L = sp.csr_matrix((f["l_val"], f["l_col"], f["l_rp"]), shape=(n, n))
    pm = f["perm"]
    assert abs(L @ L.T - A[pm][:, pm]).max() < 1e-12
    U = sp.csr_matrix((f["u_val"], f["u_col"], f["u_rp"]), shape=(n, n))
    assert abs(U - L.T).max() == 0.0


def test_cholesky_rejects_indefinite(schwz):
    rp = np.array([0, 2, 4], dtype=np.int32)
    col = np.array([0, 1, 0, 1], dtype=np.int32)
    val = np.array([1.0, 2.0, 2.0, 1.0])
    with pytest.raises(schwz.SchwzError) as e:
        schwz.cholesky(rp, col, val, True)
    assert e.value.code == schwz.capi.ERR_NOT_SPD


@pytest.mark.parametrize("case", ["lap2d", "lap3d", "ani3"])
def test_ilu0_matches_oracle_and_reproduces_pattern(schwz, oracle, case):
    """ILU(0) standing in for gko ParIlu (solve.cpp:506-532): unit-lower L, U with the
    diagonal, (L U)_ij = A_ij on the pattern of A."""
    import scipy.sparse as sp
    if case == "lap2d":
        rp, col, val = oracle.laplacian2d(17)
    elif case == "lap3d":
        rp, col, val = oracle.laplacian3d(9, 7, 5)
    else:
        g = np.load(os.path.join(G, "ani3_crop.npz"))
        rp, col, val = g["rp"], g["col"], g["val"]
    n = len(rp) - 1
    f, fo = schwz.ilu0(rp, col, val), oracle.ilu0(rp, col, val)
    for k in ("l_rp", "l_col", "u_rp", "u_col"):
        assert np.array_equal(f[k], fo[k]), k
    for k in ("l_val", "u_val"):
        assert np.array_equal(f[k], fo[k]), k   # same elimination order: bit-identical
    L = sp.csr_matrix((f["l_val"], f["l_col"], f["l_rp"]), shape=(n, n))
    U = sp.csr_matrix((f["u_val"], f["u_col"], f["u_rp"]), shape=(n, n))
    assert np.array_equal(L.diagonal(), np.ones(n))
    assert sp.tril(U, -1).nnz == 0 and sp.triu(L, 1).nnz == 0
    A = sp.csr_matrix((val, col, rp), shape=(n, n))
    pat = A.copy()
    pat.data[:] = 1.0
    assert abs((L @ U).multiply(pat) - A).max() <= 1e-13 * abs(A).max()


def test_ilu0_rejects_zero_pivot(schwz):
    rp = np.array([0, 2, 4], dtype=np.int32)
    col = np.array([0, 1, 0, 1], dtype=np.int32)
    val = np.array([0.0, 1.0, 1.0, 1.0])
    with pytest.raises(schwz.SchwzError):
        schwz.ilu0(rp, col, val)


def test_precond_names_map_like_the_reference(schwz):
    """solve.cpp:488-571: null / block-jacobi(max block size) / ilu; isai and unknown names are
    refused here (the reference only prints for unknown names)."""
    from schwz_amd import solver as sv
    code = lambda name, bs=1: sv._precond_code(schwz.Metadata(local_precond=name, precond_max_block_size=bs))
    assert code("null") == schwz.capi.PRECOND_NONE
    assert code("block-jacobi", 1) == schwz.capi.PRECOND_JACOBI
    assert code("block-jacobi", 16) == schwz.capi.PRECOND_BLOCK_JACOBI
    assert code("ilu") == schwz.capi.PRECOND_ILU
    assert code("isai") == schwz.capi.PRECOND_ISAI
    for bad in (("block-jacobi", 64), ("nope", 1)):
        with pytest.raises(schwz.capi.NotImplementedSchwz):
            code(*bad)


@pytest.mark.parametrize("case", ["lap3d", "ani3"])
def test_isai_of_ilu_factors_matches_oracle_and_inverts_on_the_pattern(schwz, oracle, case):
    """LowerIsai / UpperIsai (solve.cpp:616-638): (W T)_ij = delta_ij on the pattern of T."""
    import scipy.sparse as sp
    if case == "lap3d":
        rp, col, val = oracle.laplacian3d(9, 7, 5)
    else:
        g = np.load(os.path.join(G, "ani3_crop.npz"))
        rp, col, val = g["rp"], g["col"], g["val"]
    n = len(rp) - 1
    f = schwz.ilu0(rp, col, val)
    for name, lower in (("l", True), ("u", False)):
        trp, tcol, tval = f[name + "_rp"], f[name + "_col"], f[name + "_val"]
        w = schwz.isai(trp, tcol, tval, lower)
        wo = oracle.isai(trp, tcol, tval, lower)
        assert np.array_equal(w, wo)
        T = sp.csr_matrix((tval, tcol, trp), shape=(n, n))
        W = sp.csr_matrix((w, tcol, trp), shape=(n, n))
        pat = T.copy()
        pat.data[:] = 1.0
        assert abs((W @ T).multiply(pat) - sp.identity(n)).max() <= 1e-13


def test_local_solver_names_map_like_the_reference(schwz):
    """settings.local_solver (bench_ras.cpp:120-135): iterative-ginkgo -> CG/GMRES, direct-ginkgo
    and direct-cholmod -> own LL^T + HIP triangular solves; direct-umfpack, iterative-dealii and
    unknown names are refused."""
    from schwz_amd import solver as sv
    code = lambda name: sv._local_solver_code(schwz.Settings(local_solver=name))
    assert code("iterative-ginkgo") == schwz.capi.SOLVER_ITERATIVE
    assert code("direct-ginkgo") == schwz.capi.SOLVER_DIRECT
    assert code("direct-cholmod") == schwz.capi.SOLVER_DIRECT
    for bad in ("direct-umfpack", "iterative-dealii", "nope"):
        with pytest.raises(schwz.capi.NotImplementedSchwz):
            code(bad)


def test_csr_upload_refuses_malformed_matrices(schwz):
    """The SpMV kernels index x with the stored columns without a bounds test, so the upload
    validates row_ptr and the columns on the host -- before any device call (runs without a GPU)."""
    rp = np.array([0, 2, 4], dtype=np.int32)
    val = np.ones(4)
    for col in (np.array([0, 1, 0, 2], dtype=np.int32),      # column 2 of a 2-column matrix
                np.array([0, -1, 0, 1], dtype=np.int32)):    # negative column
        with pytest.raises(schwz.SchwzError) as e:
            schwz.Csr(rp, col, val)
        assert e.value.code == schwz.capi.ERR_INVALID
    with pytest.raises(schwz.SchwzError) as e:
        schwz.Csr(np.array([0, 3, 2], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32), np.ones(3))
    assert e.value.code == schwz.capi.ERR_INVALID


def test_partial_problem_recovers_after_a_missing_row(schwz, oracle):
    """A row source that holds part of the matrix (schwz_problem_from_rows): asking for a row it does not
    hold fails with the row id, and the handle is usable afterwards -- the miss is not remembered."""
    rp, col, val = oracle.laplacian2d(12)
    full = schwz.Problem.from_csr(rp, col, val)
    held = np.arange(30, 90, dtype=np.int64)
    part = schwz.Problem.from_rows(full.N, held, *full.extract_rows(held))
    with pytest.raises(schwz.SchwzError) as exc:
        part.extract_rows(np.array([40, 5], dtype=np.int64))
    assert "row 5" in str(exc.value)
    got = part.extract_rows(np.array([40, 41], dtype=np.int64))
    exp = full.extract_rows(np.array([40, 41], dtype=np.int64))
    for a, b in zip(got, exp):
        assert np.array_equal(a, b)
    # a subdomain that reads rows outside the part fails, one inside it still builds afterwards
    with pytest.raises(schwz.SchwzError):
        schwz.Subdomain(part, 2, 0, 2, schwz.partition_regular(full.N, 2))
    got = part.extract_rows(held[:3])
    assert np.array_equal(got[0], full.extract_rows(held[:3])[0])


# ---- the ingest boundary through the product library (ctypes): the error code, and the process survives.  The same
# ---- cases and many more run under the sanitizers in tests/test_ingest.py.

_MM = "%%MatrixMarket matrix coordinate "


def _read(schwz, tmp_path, text):
    path = tmp_path / "m.mtx"
    path.write_bytes(text.encode())
    return schwz.Problem.from_matrix_market(str(path)).to_csr()


@pytest.mark.parametrize("name,text,word", [
    ("row_index_past_n", _MM + "real general\n3 3 3\n1 1 1.0\n4 2 2.0\n3 3 3.0\n", "entry 2"),
    ("row_index_0", _MM + "real general\n3 3 3\n1 1 1.0\n0 2 2.0\n3 3 3.0\n", "entry 2"),
    ("negative_count", _MM + "real general\n3 3 -1\n1 1 1.0\n", "-1 entries"),
    ("count_beyond_the_file", _MM + "real general\n3 3 4000000000000000000\n1 1 1.0\n", "truncated"),
    ("n_beyond_32_bits", _MM + "real general\n4294967297 4294967297 1\n1 1 1.0\n", "4294967297"),
    ("complex", _MM + "complex general\n2 2 2\n1 1 2 0\n2 2 3 0\n", "\"complex\""),
    ("missing_value", _MM + "real general\n3 3 3\n1 1 1.0\n3 3 3.0\n2 2\n", "entry 3"),
    ("value_nan", _MM + "real general\n3 3 1\n1 1 nan\n", "\"nan\""),
    ("above_the_diagonal", _MM + "real symmetric\n3 3 2\n1 1 1.0\n1 2 5.0\n", "entry 2"),
    ("content_after_the_last_entry", _MM + "real general\n3 3 1\n1 1 1.0\n2 2 2.0\n", "after the last"),
])
def test_matrix_market_refusals_through_the_library(schwz, tmp_path, name, text, word):
    with pytest.raises(schwz.SchwzError) as e:
        _read(schwz, tmp_path, text)
    assert e.value.code == schwz.capi.ERR_IO and word in str(e.value)
    # the process is alive and the library still reads a file
    rp, col, val = _read(schwz, tmp_path, _MM + "real general\n1 1 1\n1 1 2.5\n")
    assert rp.tolist() == [0, 1] and col.tolist() == [0] and val.tolist() == [2.5]


def test_matrix_market_accepted_forms_through_the_library(schwz, tmp_path):
    # skew-symmetric: the mirror is -v ("symmetric" inside the word is not the symmetry)
    rp, col, val = _read(schwz, tmp_path, _MM + "real skew-symmetric\n3 3 2\n2 1 5\n3 2 7\n")
    assert rp.tolist() == [0, 1, 3, 4] and col.tolist() == [1, 0, 2, 1] and val.tolist() == [-5.0, 5.0, -7.0, 7.0]
    # symmetric with duplicates: summed in file order ((1e16 + 1) + -1e16 == 0, stored), the mirror alike
    rp, col, val = _read(schwz, tmp_path,
                         _MM + "real symmetric\n2 2 5\n1 1 1.0\n1 1 2.0\n2 1 1e16\n2 1 1.0\n2 1 -1e16\n")
    assert rp.tolist() == [0, 2, 3] and col.tolist() == [0, 1, 0] and val.tolist() == [3.0, 0.0, 0.0]
    # pattern and integer fields, mixed case, CRLF
    rp, col, val = _read(schwz, tmp_path, "%%MatrixMarket MATRIX Coordinate PATTERN General\r\n% c\r\n\r\n2 2 2\r\n2 1\r\n1 2\r\n\r\n")
    assert rp.tolist() == [0, 1, 2] and col.tolist() == [1, 0] and val.tolist() == [1.0, 1.0]
    rp, col, val = _read(schwz, tmp_path, _MM + "integer symmetric\n2 2 3\n1 1 4\n2 1 -1\n2 2 4\n")
    assert col.tolist() == [0, 1, 0, 1] and val.tolist() == [4.0, -1.0, -1.0, 4.0]


def test_problem_from_arrays_refusals_through_the_library(schwz):
    col3, val3 = np.array([0, 1, 2], dtype=np.int32), np.ones(3)
    bad = [(np.array([0, 3, 1, 2]), col3, val3),           # not monotone
           (np.array([0, -2, -1]), col3[:1], val3[:1]),   # negative
           (np.array([1, 2, 3]), col3, val3),             # does not start at 0
           (np.array([0, 1, 2, 3]), np.array([0, 3, 2], dtype=np.int32), val3),   # column >= N
           (np.array([0, 1, 2, 3]), np.array([0, -1, 2], dtype=np.int32), val3),  # column < 0
           (np.array([], dtype=np.int64), col3, val3),    # the wrapper: no row_ptr at all
           (np.array([0, 2, 4, 6]), col3, val3),          # the wrapper: col ends before row_ptr[-1]
           (np.array([0, 1, 2, 3]), col3, val3[:2])]      # the wrapper: val ends before row_ptr[-1]
    for rp, col, val in bad:
        with pytest.raises(schwz.SchwzError) as e:
            schwz.Problem.from_csr(rp, col, val)
        assert e.value.code == schwz.capi.ERR_INVALID, (rp, str(e.value))
    with pytest.raises(schwz.SchwzError) as e:
        schwz.Problem.from_rows(6, np.array([1, 3]), np.array([0, 2, 4, 6]), col3, val3)
    assert e.value.code == schwz.capi.ERR_INVALID
    with pytest.raises(schwz.SchwzError) as e:
        schwz.Problem.from_rows(6, np.array([1, 3]), np.array([0, 2, 1]), col3, val3)
    assert e.value.code == schwz.capi.ERR_INVALID
    # unsorted rows are sorted, duplicates summed in stored order, and the library is still usable
    rp, col, val = schwz.Problem.from_csr(np.array([0, 5, 6]), np.array([1, 0, 1, 0, 1, 1], dtype=np.int32),
                                          np.array([1e16, 5.0, 1.0, 7.0, -1e16, 2.0])).to_csr()
    assert rp.tolist() == [0, 2, 3] and col.tolist() == [0, 1, 1] and val.tolist() == [12.0, 0.0, 2.0]


def test_setup_and_factorization_refusals_through_the_library(schwz, oracle):
    rp, col, val = oracle.laplacian2d(6)
    prob = schwz.Problem.from_csr(rp, col, val)
    with pytest.raises(schwz.SchwzError) as e:
        schwz.Subdomain(prob, 3, 0, 2, np.array([0, 40, 20, 36], dtype=np.int64))
    assert e.value.code == schwz.capi.ERR_INVALID and "first_row" in str(e.value)
    urp = np.array([0, 1, 3, 5], dtype=np.int32)
    good = (urp, np.array([0, 0, 1, 1, 2], dtype=np.int32), np.array([2.0, -1.0, 2.0, -1.0, 2.0]))
    unsorted = (urp, np.array([0, 1, 0, 1, 2], dtype=np.int32), np.array([2.0, 2.0, -1.0, -1.0, 2.0]))
    twice = (urp, np.array([0, 1, 1, 1, 2], dtype=np.int32), np.array([2.0, 1.0, 1.0, -1.0, 2.0]))
    past = (urp, np.array([0, 0, 1, 1, 3], dtype=np.int32), np.array([2.0, -1.0, 2.0, -1.0, 2.0]))
    calls = (lambda a: schwz.cholesky(*a, True), lambda a: schwz.lu(*a, natural=True), lambda a: schwz.isai(*a, True))
    for call in calls:
        call(good)
        for rows in (unsorted, twice, past):
            with pytest.raises(schwz.SchwzError) as e:
                call(rows)
            assert e.value.code == schwz.capi.ERR_INVALID
