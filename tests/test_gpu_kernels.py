"""GPU parity of the stand-alone HIP kernels against the CPU oracle.

All calls go through the C ABI (include/schwz_hip.h).  Integer/index results
are bit-exact; fp64 results are compared with the tolerances written below
(parallel reduction order differs from the oracle's sequential sums).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL_SPMV = 1e-13   # a 7-term dot product re-associated
RTOL_CG = 1e-9      # CG iterates after tens of iterations, fp64


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("op", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 63, 1000, 100003, 524289, 1500001])   # the last two: past the launch cap, grid stride
def test_gather_scatter_ops(schwz, oracle, torch_cuda, op, n):
    torch = torch_cuda
    rng = np.random.default_rng(n + op)
    m = max(2 * n, 8)
    idx = rng.permutation(m)[:n].astype(np.int32)  # unique -> scatter is race free
    src = rng.standard_normal(m)
    into = rng.standard_normal(max(n, 1))
    # gather
    exp = oracle.gather(idx, src, into[:n].copy(), op)
    d_idx, d_src, d_into = _dev(torch, idx if n else np.zeros(1, np.int32)), _dev(torch, src), _dev(torch, into)
    schwz.gather(n, d_idx.data_ptr(), d_src.data_ptr(), d_into.data_ptr(), op)
    torch.cuda.synchronize()
    assert np.array_equal(d_into.cpu().numpy()[:n], exp)
    # scatter
    from_ = rng.standard_normal(max(n, 1))
    tgt = rng.standard_normal(m)
    exp = oracle.scatter(idx, from_[:n], tgt.copy(), op)
    d_from, d_tgt = _dev(torch, from_), _dev(torch, tgt)
    schwz.scatter(n, d_idx.data_ptr(), d_from.data_ptr(), d_tgt.data_ptr(), op)
    torch.cuda.synchronize()
    assert np.array_equal(d_tgt.cpu().numpy(), exp)


def _ragged_matrix(rng, n, max_len, long_row=None):
    """CSR with ragged rows, some empty, optionally one very long row."""
    lens = rng.integers(0, max_len + 1, size=n)
    lens[rng.integers(0, n, size=max(n // 10, 1))] = 0
    if long_row is not None:
        lens[n // 2] = min(long_row, n)
    rp = np.zeros(n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(lens)
    col = np.zeros(rp[-1], dtype=np.int32)
    for i in range(n):
        col[rp[i]:rp[i + 1]] = np.sort(rng.choice(n, size=lens[i], replace=False))
    val = rng.standard_normal(rp[-1])
    return rp, col, val


@pytest.mark.parametrize("variant", [0, 6, 7, 8, 9])
@pytest.mark.parametrize("case", ["lap2d", "lap3d", "ragged", "longrow", "tiny"])
def test_spmv_matches_oracle(schwz, oracle, torch_cuda, case, variant):
    """Every SpMV variant of the product library (0 best coding, 6 plain CSR stream kernel, 7 dictionaries,
    8 row patterns, 9 tiled kernel).  The measurement variants (1-5, 10-73, 80+) are not in libschwz_hip.so:
    test_measurement_variants_are_not_in_the_product_library."""
    torch = torch_cuda
    rng = np.random.default_rng(7)
    if case == "lap2d":
        rp, col, val = oracle.laplacian2d(97)
    elif case == "lap3d":
        rp, col, val = oracle.laplacian3d(23, 17, 11)
    elif case == "ragged":
        rp, col, val = _ragged_matrix(rng, 5000, 40)
    elif case == "longrow":
        rp, col, val = _ragged_matrix(rng, 6000, 12, long_row=5000)  # > one LDS tile
    else:
        rp, col, val = _ragged_matrix(rng, 3, 2)
    n = len(rp) - 1
    A = schwz.Csr(rp, col, val)
    x = rng.standard_normal(n)
    y0 = rng.standard_normal(n)
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)):
        exp = oracle.spmv(rp, col, val, x, alpha, beta, y0.copy())
        d_x, d_y = _dev(torch, x), _dev(torch, y0)
        A.spmv(d_x.data_ptr(), d_y.data_ptr(), alpha, beta, variant=variant)
        torch.cuda.synchronize()
        got = d_y.cpu().numpy()
        scale = np.abs(exp).max() + 1e-300
        assert np.abs(got - exp).max() <= RTOL_SPMV * max(scale, 1.0) * 50


@pytest.mark.gpu
def test_measurement_variants_are_not_in_the_product_library(schwz, oracle, torch_cuda):
    """tools/probes/spmv_variants.hip and the ablation builds of spmv_stream.hip are linked into
    libschwz_hip_probes.so only; the product library refuses their variant ids and says where they live."""
    torch = torch_cuda
    if "probes" in os.path.basename(schwz.capi.LIB_PATH):
        pytest.skip("running on the measurement build")
    rp, col, val = oracle.laplacian2d(20)
    A = schwz.Csr(rp, col, val)
    x = _dev(torch, np.ones(400))
    y = _dev(torch, np.zeros(400))
    for variant in (1, 2, 3, 4, 5, 10, 80, 208):
        with pytest.raises(schwz.SchwzError) as exc:
            A.spmv(x.data_ptr(), y.data_ptr(), 1.0, 0.0, variant=variant)
        assert "libschwz_hip_probes.so" in str(exc.value)


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [5, 8, 13, 16, 30, 32, 40])
def test_plain_csr_stream_kernel_is_bit_identical_to_the_tiled_kernel(schwz, oracle, torch_cuda, monkeypatch, max_len):
    """The straight-line plain-CSR kernel (spmv_stream.hip, variants 0 / 6 on matrices whose rows hold at most
    32 entries) against spmv_tiled2_kernel (variant 9): same tiles, same products, same summation order, same
    grid -- y bit for bit, and so the stored-q CG built on its fused modes (start residual, q = A p with the
    partial p.q).  Ragged rows with empty ones (masked-add counts 8 / 16 / 32; rows of 40 keep the tiled
    kernel), stencils with odd plane sizes, a matrix with a single tile."""
    torch = torch_cuda
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "0")
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "0")
    monkeypatch.setenv("SCHWZ_SPMV_DICT", "0")
    rng = np.random.default_rng(100 + max_len)
    mats = [_ragged_matrix(rng, 7001, max_len), _ragged_matrix(rng, 130, max_len)]
    if max_len == 8:
        mats += [oracle.laplacian3d(37, 29, 23), oracle.laplacian2d(211)]
    for rp, col, val in mats:
        n = len(rp) - 1
        A = schwz.Csr(rp, col, val)
        assert A.format() == 0
        x = rng.standard_normal(n)
        d_x = _dev(torch, x)
        ys = []
        for variant in (6, 9, 0):
            d_y = _dev(torch, np.zeros(n))
            A.spmv(d_x.data_ptr(), d_y.data_ptr(), 1.0, 0.0, variant=variant)
            torch.cuda.synchronize()
            ys.append(d_y.cpu().numpy())
        assert np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2])
        exp = oracle.spmv(rp, col, val, x, 1.0, 0.0, np.zeros(n))
        assert np.abs(ys[0] - exp).max() <= RTOL_SPMV * max(np.abs(exp).max(), 1.0) * 50
    # the fused modes through CG on an SPD matrix (stored-q iteration: kSpmvResidInit, kSpmvDot)
    rp, col, val = oracle.laplacian3d(37, 29, 23)
    n = len(rp) - 1
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)
    A = schwz.Csr(rp, col, val)
    assert A.format() == 0
    cg = schwz.Pcg(A, 1)
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 25)
    assert it == 25 and cg.flavour() & 3 == 0
    got = d_x.cpu().numpy()
    exp, _, _ = oracle.pcg(rp, col, val, b, x0, 1, 0.0, 25)
    assert np.abs(got - exp).max() <= RTOL_CG * np.abs(exp).max()


def test_plain_csr_stream_kernel_on_wide_planes(schwz, torch_cuda, monkeypatch):
    """Planes of more than 2048 tiles (1024 x 1024): the stream kernel walks an explicit per-XCD tile sequence
    (sub-stripes of 128 tiles through all planes, CsrView::stream_order) instead of the block-cyclic deal, in
    short-lived workgroups.  Every tile exactly once: y bit for bit the tiled kernel's (variant 9), with the
    sequence switched off as well, and the fused modes through three CG iterations on plain CSR."""
    torch = torch_cuda
    for k in ("SCHWZ_SPMV_PAIR", "SCHWZ_SPMV_PATTERN", "SCHWZ_SPMV_DICT"):
        monkeypatch.setenv(k, "0")
    shape = (1024, 1024, 9)
    prob = schwz.Problem.laplacian(3, *shape)
    sd = schwz.Subdomain(prob, 1, 0, 2, schwz.partition_regular(prob.N, 1))
    rp, col, val = sd.local_matrix()
    n = len(rp) - 1
    x = torch.randn(n, dtype=torch.float64, device="cuda")
    b = torch.randn(n, dtype=torch.float64, device="cuda")
    ys, sols = {}, {}
    for order in ("1", "0"):
        monkeypatch.setenv("SCHWZ_STREAM_ORDER", order)
        A = schwz.Csr(rp, col, val)
        assert A.format() == 0
        for variant in (6, 9):
            y = torch.zeros(n, dtype=torch.float64, device="cuda")
            A.spmv(x.data_ptr(), y.data_ptr(), 1.0, 0.0, variant=variant)
            torch.cuda.synchronize()
            ys[(order, variant)] = y
        # start residual + q = A p with the fused dots (per-workgroup partial sums folded in another order)
        cg = schwz.Pcg(A, 1)
        xs = torch.zeros(n, dtype=torch.float64, device="cuda")
        it, rn = cg.solve(b.data_ptr(), xs.data_ptr(), 0.0, 3)
        assert it == 3
        sols[order] = xs
        del cg, A
    ref = ys[("1", 9)]
    for k, y in ys.items():
        assert torch.equal(y, ref), k
    assert float((sols["1"] - sols["0"]).abs().max()) <= 1e-12 * float(sols["0"].abs().max())


def test_spmv_is_reproducible(schwz, oracle, torch_cuda):
    torch = torch_cuda
    rp, col, val = oracle.laplacian3d(40)
    A = schwz.Csr(rp, col, val)
    x = _dev(torch, np.random.default_rng(1).standard_normal(len(rp) - 1))
    y1, y2 = torch.zeros_like(x), torch.zeros_like(x)
    A.spmv(x.data_ptr(), y1.data_ptr())
    A.spmv(x.data_ptr(), y2.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("case", ["lap2d", "lap3d", "ani3"])
def test_pcg_fixed_iterations_match_oracle(schwz, oracle, torch_cuda, case, precond):
    """rtol=0: exactly max_iters updates on both sides; iterates must agree."""
    torch = torch_cuda
    if case == "lap2d":
        rp, col, val = oracle.laplacian2d(64)
    elif case == "lap3d":
        rp, col, val = oracle.laplacian3d(20, 20, 20)
    else:
        g = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "ani3_crop.npz"))
        rp, col, val = g["rp"], g["col"], g["val"]
    n = len(rp) - 1
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n) * 0.1
    A = schwz.Csr(rp, col, val)
    cg = schwz.Pcg(A, precond)
    for iters in (1, 7, 30):
        exp, it_o, rn_o = oracle.pcg(rp, col, val, b, x0, precond, 0.0, iters)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it_g, rn_g = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, iters)
        got = d_x.cpu().numpy()
        assert it_g == it_o == iters
        assert np.abs(got - exp).max() <= RTOL_CG * np.abs(exp).max()
        assert abs(rn_g - rn_o) <= 1e-8 * max(rn_o, 1e-300) + 1e-14


@pytest.mark.parametrize("precond", [0, 1])
def test_pcg_tolerance_stop_matches_oracle(schwz, oracle, torch_cuda, precond):
    """Residual-reduction stop: same iteration count and solution."""
    torch = torch_cuda
    rp, col, val = oracle.laplacian2d(48)
    n = len(rp) - 1
    b = np.ones(n)
    A = schwz.Csr(rp, col, val)
    cg = schwz.Pcg(A, precond)
    for rtol in (1e-2, 1e-6, 1e-12):
        exp, it_o, rn_o = oracle.pcg(rp, col, val, b, None, precond, rtol, n)
        d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
        it_g, rn_g = cg.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, n)
        got = d_x.cpu().numpy()
        assert abs(it_g - it_o) <= 1, (it_g, it_o)
        assert np.abs(got - exp).max() <= 1e-7 * np.abs(exp).max()


def test_pcg_zero_rhs_stops_immediately(schwz, oracle, torch_cuda):
    torch = torch_cuda
    rp, col, val = oracle.laplacian2d(8)
    n = len(rp) - 1
    A = schwz.Csr(rp, col, val)
    cg = schwz.Pcg(A, 1)
    d_b = torch.zeros(n, dtype=torch.float64, device="cuda")
    d_x = torch.zeros(n, dtype=torch.float64, device="cuda")
    it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 5)
    assert it == 0 and rn == 0.0
    assert not torch.isnan(d_x).any()


@pytest.mark.parametrize("natural", [True, False])
@pytest.mark.parametrize("case", ["lap2d", "ani3"])
def test_direct_solve_matches_oracle(schwz, oracle, torch_cuda, case, natural):
    """Own LL^T + level-scheduled HIP tri-solves vs the oracle's factor+solve."""
    torch = torch_cuda
    import os
    if case == "lap2d":
        rp, col, val = oracle.laplacian2d(24)
    else:
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ani3_crop.npz"))
        rp, col, val = g["rp"], g["col"], g["val"]
    n = len(rp) - 1
    f = schwz.cholesky(rp, col, val, natural)
    fo = oracle.cholesky(rp, col, val, natural)
    # identical ordering rule and arithmetic order per column up to rounding
    assert np.array_equal(f["perm"], fo["perm"])
    assert np.array_equal(f["l_rp"], fo["l_rp"]) and np.array_equal(f["l_col"], fo["l_col"])
    assert np.abs(f["l_val"] - fo["l_val"]).max() <= 1e-12 * np.abs(fo["l_val"]).max()
    b = np.random.default_rng(5).standard_normal(n)
    exp = oracle.direct_solve(fo, b)
    trs = schwz.Trs(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"], f["perm"])
    d_b = _dev(torch, b)
    d_y = torch.zeros(n, dtype=torch.float64, device="cuda")
    trs.solve(d_b.data_ptr(), d_y.data_ptr())
    torch.cuda.synchronize()
    got = d_y.cpu().numpy()
    assert np.abs(got - exp).max() <= 1e-10 * np.abs(exp).max()


@pytest.mark.parametrize("pc", [(2, 2), (2, 7), (2, 16), (2, 32), (3, 1), (4, 1)])
@pytest.mark.parametrize("case", ["lap2d", "lap3d", "ani3", "nodes3"])
def test_pcg_block_jacobi_and_ilu_match_oracle(schwz, oracle, torch_cuda, case, pc):
    """Block-Jacobi (gko preconditioner::Jacobi, solve.cpp:488-504: blocks found by supervariable
    agglomeration -- consecutive blocks on the stencil matrices, whole 3-unknown nodes per block,
    i.e. blocks of different sizes, on `nodes3`) and ILU(0) (solve.cpp:506-532) in the device-resident
    PCG against the oracle's recurrence."""
    torch = torch_cuda
    precond, bs = pc
    if case == "nodes3":
        if precond != 2:
            pytest.skip("ILU(0) is exact on this block-tridiagonal matrix: CG is done after two iterations")
        import scipy.sparse as sp
        t = sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(900, 900), format="csr")
        blk = np.array([[2.0, 0.3, 0.1], [0.3, 1.5, 0.2], [0.1, 0.2, 1.8]])   # SPD: rows of a node share their pattern
        a = sp.kron(t, blk, format="csr")
        a.sort_indices()
        rp, col, val = a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.copy()
        if precond == 2 and bs in (7, 16, 32):
            ptr = oracle.jacobi_blocks(rp, col, bs)
            assert set(np.diff(ptr)) <= {3 * (bs // 3), len(rp) - 1 - ptr[-2]} and (np.diff(ptr) % 3 == 0).all()
    elif case == "lap2d":
        rp, col, val = oracle.laplacian2d(50)
    elif case == "lap3d":
        rp, col, val = oracle.laplacian3d(21, 19, 23)   # n = 9177 > 8192: multi-launch trs plan
    else:
        g = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "ani3_crop.npz"))
        rp, col, val = g["rp"], g["col"], g["val"]
    n = len(rp) - 1
    rng = np.random.default_rng(17)
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n) * 0.1
    A = schwz.Csr(rp, col, val)
    cg = schwz.Pcg(A, precond, bs)
    for iters in (1, 6, 25):
        exp, it_o, rn_o = oracle.pcg(rp, col, val, b, x0, precond, 0.0, iters, block_size=bs)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it_g, rn_g = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, iters)
        got = d_x.cpu().numpy()
        assert it_g == it_o == iters
        assert np.abs(got - exp).max() <= RTOL_CG * np.abs(exp).max()
        assert abs(rn_g - rn_o) <= 1e-8 * max(rn_o, 1e-300) + 1e-14
    # tolerance stop
    exp, it_o, rn_o = oracle.pcg(rp, col, val, b, None, precond, 1e-10, n, block_size=bs)
    d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
    it_g, rn_g = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 1e-10, n)
    assert abs(it_g - it_o) <= 1, (it_g, it_o)
    assert np.abs(d_x.cpu().numpy() - exp).max() <= 1e-7 * np.abs(exp).max()


@pytest.mark.parametrize("pc", [(2, 7), (2, 32), (4, 1)])
def test_pcg_block_jacobi_and_isai_past_the_grid_cap(schwz, oracle, torch_cuda, pc):
    """Block-Jacobi (block sizes 7 and 32) and ISAI applications on n = 725^2 = 525 625 > 524 288 rows: the
    preconditioner kernels run with a capped grid and stride.  Three fixed iterations against the oracle's
    recurrence, at the tolerance of test_pcg_block_jacobi_and_ilu_match_oracle."""
    torch = torch_cuda
    precond, bs = pc
    rp, col, val = oracle.laplacian2d(725)
    n = len(rp) - 1
    assert n > 2048 * 256
    rng = np.random.default_rng(19)
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n) * 0.1
    A = schwz.Csr(rp, col, val)
    cg = schwz.Pcg(A, precond, bs)
    exp, it_o, rn_o = oracle.pcg(rp, col, val, b, x0, precond, 0.0, 3, block_size=bs)
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    it_g, rn_g = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 3)
    got = d_x.cpu().numpy()
    assert it_g == it_o == 3
    assert np.abs(got - exp).max() <= RTOL_CG * np.abs(exp).max()
    assert abs(rn_g - rn_o) <= 1e-8 * max(rn_o, 1e-300) + 1e-14


@pytest.mark.parametrize("pc", [(0, 1), (1, 1), (2, 8), (3, 1), (4, 1)])
@pytest.mark.parametrize("restart", [1, 4, 30])
def test_gmres_matches_oracle(schwz, oracle, torch_cuda, convdiff, restart, pc):
    """Device-resident GMRES(restart), right preconditioned (solve.cpp:486-520), against the
    oracle's restatement on a non-symmetric convection-diffusion matrix: fixed numbers of Krylov
    vectors (rtol = 0) give the same iterate, a tolerance stop the same count."""
    torch = torch_cuda
    precond, bs = pc
    rp, col, val = convdiff(40)
    n = len(rp) - 1
    rng = np.random.default_rng(29)
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n) * 0.1
    A = schwz.Csr(rp, col, val)
    gm = schwz.Gmres(A, precond, bs, restart)
    for iters in (1, 5, 23):
        exp, it_o, rn_o = oracle.gmres(rp, col, val, b, x0, precond, 0.0, iters, restart, bs)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it_g, rn_g = gm.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, iters)
        got = d_x.cpu().numpy()
        assert it_g == it_o == iters
        assert np.abs(got - exp).max() <= 1e-9 * np.abs(exp).max()
        assert abs(rn_g - rn_o) <= 1e-8 * rn_o
    exp, it_o, rn_o = oracle.gmres(rp, col, val, b, None, precond, 1e-9, 4000, restart, bs)
    d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
    it_g, rn_g = gm.solve(d_b.data_ptr(), d_x.data_ptr(), 1e-9, 4000)
    assert abs(it_g - it_o) <= max(1, restart // 8), (it_g, it_o)
    assert np.abs(d_x.cpu().numpy() - exp).max() <= 1e-6 * np.abs(exp).max()
    # zero right-hand side: no iteration, x untouched
    d_b = torch.zeros(n, dtype=torch.float64, device="cuda")
    d_x = torch.zeros(n, dtype=torch.float64, device="cuda")
    it_g, rn_g = gm.solve(d_b.data_ptr(), d_x.data_ptr(), 1e-9, 50)
    assert it_g == 0 and rn_g == 0.0 and not d_x.cpu().numpy().any()


@pytest.mark.parametrize("kind", ["ilu_noperm", "chol_perm"])
def test_triangular_solves_multi_launch_plan(schwz, oracle, torch_cuda, monkeypatch, kind):
    """n > 8192 rows: the level schedule runs as wide/narrow segment launches instead of the
    single-workgroup kernel; same answer as the oracle's sequential sweeps."""
    torch = torch_cuda
    import scipy.sparse as sp
    import scipy.sparse.linalg as sl
    rp, col, val = oracle.laplacian3d(27, 25, 22)
    n = len(rp) - 1
    assert n > 8192
    b = np.random.default_rng(23).standard_normal(n)
    if kind == "ilu_noperm":
        f = schwz.ilu0(rp, col, val)
        L = sp.csr_matrix((f["l_val"], f["l_col"], f["l_rp"]), shape=(n, n))
        U = sp.csr_matrix((f["u_val"], f["u_col"], f["u_rp"]), shape=(n, n))
        exp = sl.spsolve_triangular(U, sl.spsolve_triangular(L, b, lower=True), lower=False)
        perm = None
    else:
        f = schwz.cholesky(rp, col, val, False)
        fo = oracle.cholesky(rp, col, val, False)
        exp = oracle.direct_solve(fo, b)
        perm = f["perm"]
    trs = schwz.Trs(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"], perm)
    d_b = _dev(torch, b)
    d_y = torch.zeros(n, dtype=torch.float64, device="cuda")
    for _ in range(2):   # second call reuses the plan and work vectors
        trs.solve(d_b.data_ptr(), d_y.data_ptr())
    torch.cuda.synchronize()
    got = d_y.cpu().numpy()
    assert np.abs(got - exp).max() <= 1e-10 * np.abs(exp).max()
    # in place (b == y) is allowed, like gko apply(b, b) in solve.cpp:709-720
    trs.solve(d_b.data_ptr(), d_b.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_b.cpu().numpy(), got)
    # the flag-driven sweeps (one persistent launch per factor, rows hand over through the solution
    # vector) and the level-by-level launch plan sum every row in the same order: the same bits
    monkeypatch.setenv("SCHWZ_TRS_FLAGS", "0")
    plan = schwz.Trs(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"], perm)
    d_b2, d_y2 = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
    for _ in range(3):
        plan.solve(d_b2.data_ptr(), d_y2.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_y2.cpu().numpy(), got)


@pytest.mark.parametrize("case", ["lap3d", "ragged"])
def test_spmv_with_forced_tile_order(schwz, oracle, torch_cuda, case, monkeypatch):
    """The BFS visiting order of the row tiles (a locality permutation of the launch schedule,
    not of the data) must not change a single bit of the result."""
    torch = torch_cuda
    rng = np.random.default_rng(11)
    if case == "lap3d":
        rp, col, val = oracle.laplacian3d(31, 29, 23)
    else:
        rp, col, val = _ragged_matrix(rng, 20000, 24, long_row=3000)
    n = len(rp) - 1
    x = _dev(torch, rng.standard_normal(n))
    ys = []
    for mode in ("0", "2"):
        monkeypatch.setenv("SCHWZ_TILE_ORDER", mode)
        A = schwz.Csr(rp, col, val)
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        A.spmv(x.data_ptr(), y.data_ptr())
        torch.cuda.synchronize()
        ys.append(y.cpu().numpy())
    assert np.array_equal(ys[0], ys[1])
    exp = oracle.spmv(rp, col, val, x.cpu().numpy())
    assert np.abs(ys[1] - exp).max() <= 1e-12 * max(np.abs(exp).max(), 1.0)


def _mixed_matrix(oracle, rng):
    """Laplacian rows (few distinct values/offsets -> dictionary tiles), then rows with random
    values (raw tiles), one row longer than a tile, empty rows."""
    rp1, col1, val1 = oracle.laplacian3d(20, 15, 12)
    n1 = len(rp1) - 1
    rp2, col2, val2 = _ragged_matrix(rng, 3000, 20, long_row=2500)
    n = n1 + 3000
    rp = np.concatenate([rp1, rp1[-1] + rp2[1:]]).astype(np.int32)
    col = np.concatenate([col1, col2 + rng.integers(0, n1)]).astype(np.int32) % n
    # keep columns sorted within the random rows
    for i in range(n1, n):
        col[rp[i]:rp[i + 1]] = np.sort(col[rp[i]:rp[i + 1]])
    val = np.concatenate([val1, val2])
    return rp, col, val


@pytest.mark.parametrize("case", ["lap3d_even", "lap3d_odd_rows", "lap2d", "ani3_forced", "mixed_forced",
                                  "unsorted_rows"])
def test_row_pair_coding_is_bit_identical_to_plain_csr(schwz, oracle, torch_cuda, monkeypatch, case):
    """The row-pair coding (spmv_pair.hip, the default for stencil-like matrices): y = alpha A x +
    beta y bit for bit equal to the plain CSR kernel and to the row-pattern kernel -- full and
    partial last chunks, odd row counts (a pair without a second row), chunks that fall back to
    CSR rows, the safe path near the first / last column -- and the fused epilogues through a
    CG solve against the oracle.  Rows with unsorted columns must not be pair coded at all."""
    torch = torch_cuda
    rng = np.random.default_rng(31)
    want = 3
    if case == "lap3d_even":
        rp, col, val = oracle.laplacian3d(64, 64, 40)
    elif case == "lap3d_odd_rows":
        rp, col, val = oracle.laplacian3d(45, 41, 39)     # 71955 rows: odd, partial last chunk
    elif case == "lap2d":
        rp, col, val = oracle.laplacian2d(301)
    elif case == "ani3_forced":
        monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
        monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
        g = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "ani3_crop.npz"))
        rp, col, val = g["rp"], g["col"], g["val"]
    elif case == "mixed_forced":
        monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
        monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
        rp, col, val = _mixed_matrix(oracle, rng)
    else:
        rp, col, val = oracle.laplacian3d(40, 40, 40)
        col, val = col.copy(), val.copy()
        for i in range(0, len(rp) - 1, 7):               # swap two entries: same matrix, unsorted rows
            s, e = rp[i], rp[i + 1]
            if e - s >= 2:
                col[s], col[s + 1] = col[s + 1], col[s]
                val[s], val[s + 1] = val[s + 1], val[s]
        want = None
    n = len(rp) - 1
    A = schwz.Csr(rp, col, val)
    if want is None:
        assert A.format() != 3
    else:
        assert A.format() == want
    x = _dev(torch, rng.standard_normal(n))
    y0 = _dev(torch, rng.standard_normal(n))
    for alpha, beta in ((1.0, 0.0), (-0.75, 2.5)):
        ys = {}
        for v in (0, 8, 6):
            ys[v] = y0.clone()
            A.spmv(x.data_ptr(), ys[v].data_ptr(), alpha, beta, v)
        torch.cuda.synchronize()
        assert torch.equal(ys[0], ys[6]) and torch.equal(ys[8], ys[6])
    exp = oracle.spmv(rp, col, val, x.cpu().numpy())
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    A.spmv(x.data_ptr(), y.data_ptr())
    assert np.abs(y.cpu().numpy() - exp).max() <= 1e-12 * max(np.abs(exp).max(), 1.0)
    if case in ("lap3d_even", "lap3d_odd_rows", "lap2d"):
        b = rng.standard_normal(n)
        cg = schwz.Pcg(A, 1)
        expx, it_o, rn_o = oracle.pcg(rp, col, val, b, None, 1, 0.0, 12)
        d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
        it_g, rn_g = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 12)
        assert it_g == it_o == 12
        assert np.abs(d_x.cpu().numpy() - expx).max() <= RTOL_CG * np.abs(expx).max()
        assert abs(rn_g - rn_o) <= 1e-8 * rn_o


def test_coded_tiles_are_bit_identical_to_plain_csr(schwz, oracle, torch_cuda, monkeypatch):
    """Variant 0 (row-pattern coded tiles), variant 7 (per-entry dictionary tiles) and variant 6
    (plain CSR) sum the same individually rounded products in the same order => identical bits,
    on a matrix that mixes codable tiles, raw tiles, a long row and empty rows, and for every
    epilogue the PCG uses (checked through a short solve)."""
    torch = torch_cuda
    rng = np.random.default_rng(21)
    monkeypatch.setenv("SCHWZ_SPMV_DICT", "2")     # code whatever can be coded, whatever the share
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
    rp, col, val = _mixed_matrix(oracle, rng)
    n = len(rp) - 1
    A = schwz.Csr(rp, col, val)
    x = _dev(torch, rng.standard_normal(n))
    ys = {}
    for v in (0, 7, 6):
        ys[v] = torch.zeros(n, dtype=torch.float64, device="cuda")
        A.spmv(x.data_ptr(), ys[v].data_ptr(), 1.0, 0.0, v)
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[6]) and torch.equal(ys[7], ys[6])
    exp = oracle.spmv(rp, col, val, x.cpu().numpy())
    assert np.abs(ys[0].cpu().numpy() - exp).max() <= 1e-12 * max(np.abs(exp).max(), 1.0)
    # matrices that are entirely coded: CG trajectories must coincide bit for bit (with p.(A p)
    # summed over full rows: the upper-triangle form of symmetric pair-coded matrices rounds differently)
    monkeypatch.setenv("SCHWZ_SPMV_SYM", "0")
    rp, col, val = oracle.laplacian3d(33, 21, 17)
    n = len(rp) - 1
    b = rng.standard_normal(n)
    sols = []
    for pat_env, dict_env in (("1", "1"), ("0", "1"), ("0", "0")):
        monkeypatch.setenv("SCHWZ_SPMV_PATTERN", pat_env)
        monkeypatch.setenv("SCHWZ_SPMV_DICT", dict_env)
        A = schwz.Csr(rp, col, val)
        cg = schwz.Pcg(A, 1)
        d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 25)
        sols.append((d_x.cpu().numpy(), rn))
    for k in (1, 2):
        assert np.array_equal(sols[0][0], sols[k][0]) and sols[0][1] == sols[k][1]


@pytest.mark.parametrize("nvalues", [1, 5, 40])
def test_qfree_cg_with_every_diagonal_representation(schwz, oracle, torch_cuda, monkeypatch, nvalues):
    """The q-free CG iteration of row-pair coded matrices (q = A p recomputed inside the update
    launch) with the Jacobi diagonal as a scalar (1 distinct value) and as the full vector (5 or
    40 values: a pair-coded matrix never gets 1-byte diagonal codes, which would select the
    slower stored-q iteration); each against the oracle."""
    torch = torch_cuda
    rp, col, val = oracle.laplacian3d(40, 40, 40)
    n = len(rp) - 1
    val = val.copy()
    shifts = np.linspace(0.0, 2.0, nvalues) if nvalues > 1 else np.zeros(1)
    rows = np.repeat(np.arange(n), np.diff(rp))
    diag = col == rows
    val[diag] += shifts[(rows[diag] // 4096) % nvalues]   # piecewise constant: few pairs per chunk
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")   # code it whatever the table sharing heuristics say
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
    A = schwz.Csr(rp, col, val)
    assert A.format() == 3
    rng = np.random.default_rng(13)
    b = rng.standard_normal(n)
    x0 = rng.standard_normal(n) * 0.1
    cg = schwz.Pcg(A, 1)
    for iters in (1, 9, 30):
        exp, it_o, rn_o = oracle.pcg(rp, col, val, b, x0, 1, 0.0, iters)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it_g, rn_g = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, iters)
        assert it_g == it_o == iters
        assert np.abs(d_x.cpu().numpy() - exp).max() <= RTOL_CG * np.abs(exp).max()
        assert abs(rn_g - rn_o) <= 1e-8 * rn_o
    exp, it_o, rn_o = oracle.pcg(rp, col, val, b, None, 1, 1e-9, n)
    d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
    it_g, rn_g = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 1e-9, n)
    assert abs(it_g - it_o) <= 1 and np.abs(d_x.cpu().numpy() - exp).max() <= 1e-7 * np.abs(exp).max()


def _symmetric_test_matrix(oracle, rng, rough, shifted=True):
    """40^3 Laplacian, `shifted`: with a piecewise-constant diagonal shift (several pair tables);
    `rough`: a band of rows gets random symmetric couplings, so its chunks stay plain CSR rows."""
    import scipy.sparse as sp
    rp, col, val = oracle.laplacian3d(40, 40, 40)
    n = len(rp) - 1
    M = sp.csr_matrix((val, col, rp), shape=(n, n))
    U = sp.triu(M, 1).tocoo()
    data = U.data.copy()
    if rough:
        band = (U.row >= 20000) & (U.row < 23000)
        data[band] *= 1.0 - 0.5 * rng.random(int(band.sum()))  # weaker couplings: still diagonally dominant
    U = sp.coo_matrix((data, (U.row, U.col)), shape=(n, n)).tocsr()
    diag = M.diagonal() + (3.0 * ((np.arange(n) // 4096) % 5) / 5.0 if shifted else 0.0)
    S = (sp.diags(diag) + U + U.T).tocsr()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy()


@pytest.mark.parametrize("diag", ["uniform", "vector"])
@pytest.mark.parametrize("rough", [False, True])
def test_symmetric_matrices_take_the_dot_from_the_upper_triangle(schwz, oracle, torch_cuda, monkeypatch, rough, diag):
    """A pair-coded matrix that the upload finds symmetric bit for bit gets upper-triangle tables,
    and the q-free CG iteration takes p.(A p) = sum_i p_i (a_ii p_i + 2 sum_{j>i} a_ij p_j) from
    them (kSpmvDotSym): same iterates as the oracle within the CG tolerance, and as the full-row
    form (SCHWZ_SPMV_SYM=0) to rounding.  One changed value or one missing mirror entry and the
    matrix is not symmetric: no tables, and the result is the full-row one bit for bit.
    Run with the Jacobi diagonal as a scalar (`uniform`), as a full vector (`vector`; as 1-byte
    codes the iteration keeps a stored q and never takes this launch) or absent (precond 0).
    Systems of this size (launch bound) run two launches per iteration: the direction update and
    the next p.(A p) are one (kSpmvDirDotSym, the new p recomputed at every gathered neighbour)."""
    import ctypes
    torch = torch_cuda
    rng = np.random.default_rng(77)
    rp, col, val = _symmetric_test_matrix(oracle, rng, rough, shifted=diag == "vector")
    n = len(rp) - 1
    if diag == "vector":
        monkeypatch.setenv("SCHWZ_DIAG_DICT", "0")   # 5 distinct values would otherwise become 1-byte codes
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)

    def solve(rp_, col_, val_, iters, rtol=0.0, precond=1):
        A = schwz.Csr(rp_, col_, val_)
        assert A.format() == 3
        cg = schwz.Pcg(A, precond)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, iters)
        return A.symmetric(), it, rn, d_x.cpu().numpy()

    for precond in (1, 0):
        for iters in (1, 2, 30):
            # the q-free iteration ran: its update launch is the one the profiling hook files as kind 1;
            # kind 0 counts the p.(A p) launches inside the iteration: every one, or -- fused with the
            # direction update -- all but the last iteration's (the first of a solve runs outside)
            schwz.capi.check(schwz.capi.lib.schwz_profile_begin(4 * iters + 8))
            sym, it, rn, x = solve(rp, col, val, iters, precond=precond)
            tot, launches = ctypes.c_double(0.0), ctypes.c_int64(0)
            schwz.capi.check(schwz.capi.lib.schwz_profile_end(ctypes.byref(tot), ctypes.byref(launches)))
            upd_ms, upd = ctypes.c_double(0.0), ctypes.c_int64(0)
            schwz.capi.check(schwz.capi.lib.schwz_profile_kind(1, ctypes.byref(upd_ms), ctypes.byref(upd)))
            fused = os.environ.get("SCHWZ_CG_FUSEDIR", "1")[:1] != "0" and os.environ.get("SCHWZ_CG_SYM", "1")[:1] != "0"
            assert sym and launches.value == (iters - 1 if fused else iters)
            if os.environ.get("SCHWZ_CG_QFREE", "1")[:1] != "0":
                assert upd.value == iters
            exp, it_o, rn_o = oracle.pcg(rp, col, val, b, x0, precond, 0.0, iters)
            assert it == it_o == iters
            assert np.abs(x - exp).max() <= RTOL_CG * np.abs(exp).max()
            assert abs(rn - rn_o) <= 1e-8 * rn_o
    sym, it, rn, x = solve(rp, col, val, 30)
    # to convergence, with the stopping test on
    sym, it_c, rn_c, x_c = solve(rp, col, val, n, 1e-9)
    exp_c, it_oc, _ = oracle.pcg(rp, col, val, b, x0, 1, 1e-9, n)
    assert abs(it_c - it_oc) <= 1 and np.abs(x_c - exp_c).max() <= 1e-7 * np.abs(exp_c).max()
    # the full-row form of the same matrix
    monkeypatch.setenv("SCHWZ_SPMV_SYM", "0")
    sym_f, _, rn_f, x_f = solve(rp, col, val, 30)
    assert not sym_f
    assert np.abs(x - x_f).max() <= 1e-11 * np.abs(x_f).max()
    monkeypatch.delenv("SCHWZ_SPMV_SYM")
    # one value off its mirror image
    val2 = val.copy()
    j = rp[12345] + 1
    assert col[j] != 12345
    val2[j] *= 1.0 + 2.0 ** -40
    sym2, _, rn2, x2 = solve(rp, col, val2, 30)
    assert not sym2
    monkeypatch.setenv("SCHWZ_SPMV_SYM", "0")
    _, _, rn2f, x2f = solve(rp, col, val2, 30)
    assert np.array_equal(x2, x2f) and rn2 == rn2f
    monkeypatch.delenv("SCHWZ_SPMV_SYM")
    # one entry without its mirror entry (row 777 loses its last coupling)
    keep = np.ones(len(col), dtype=bool)
    keep[rp[778] - 1] = False
    assert col[rp[778] - 1] > 777
    rp3 = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(n), np.diff(rp))[keep], minlength=n))])
    sym3, _, _, x3 = solve(rp3.astype(np.int32), col[keep], val[keep], 10)
    assert not sym3
    exp3, _, _ = oracle.pcg(rp3.astype(np.int32), col[keep], val[keep], b, x0, 1, 0.0, 10)
    assert np.abs(x3 - exp3).max() <= RTOL_CG * np.abs(exp3).max()


@pytest.mark.parametrize("nshift", [1, 3, 40])
def test_pcg_diagonal_representations_agree(schwz, oracle, torch_cuda, monkeypatch, nshift):
    """Jacobi 1/diag as a scalar (1 distinct value), as 1-byte codes into a dictionary (3), or as
    the full vector (40 distinct -> no coding): identical bits to the forced full-vector run, and
    the oracle's iterates within tolerance.  n is odd to exercise the tail element.  Row-pair
    coding is switched off: pair-coded matrices always keep the full vector."""
    torch = torch_cuda
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "0")
    rp, col, val = oracle.laplacian2d(21)  # 441 rows
    n = len(rp) - 1
    val = val.copy()
    shifts = np.linspace(0.0, 1.0, nshift) if nshift > 1 else np.zeros(1)
    for i in range(n):
        for j in range(rp[i], rp[i + 1]):
            if col[j] == i:
                val[j] += shifts[i % nshift]
    b = np.random.default_rng(9).standard_normal(n)
    res = []
    for env in ("1", "0"):
        monkeypatch.setenv("SCHWZ_DIAG_DICT", env)
        A = schwz.Csr(rp, col, val)
        cg = schwz.Pcg(A, 1)
        d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 15)
        res.append((d_x.cpu().numpy(), rn))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    exp, _, rn_o = oracle.pcg(rp, col, val, b, None, 1, 0.0, 15)
    assert np.abs(res[0][0] - exp).max() <= RTOL_CG * np.abs(exp).max()


@pytest.mark.parametrize("coding", ["pairs", "plain_csr", "dictionary"])
@pytest.mark.parametrize("n_edge", [(24, 20, 17), (21, 19, 15)])
def test_deferred_x_update_is_bit_identical(schwz, oracle, torch_cuda, monkeypatch, n_edge, coding):
    """Large systems keep x out of the CG iteration: the search directions of up to 16 iterations
    stay in a ring, the update launch stores alpha_k, and one launch per full ring (and one at the
    end) applies x += sum alpha_k p_k in iteration order -- in the q-free iteration of row-pair coded matrices
    and in the stored-q iteration of the others (one more ring vector: q is in use).  Forced on a small system here
    (SCHWZ_CG_DEFERX=2) and compared bit for bit with the iteration that updates x itself: fixed
    iteration counts around the ring length, a tolerance stop inside a ring, even and odd n."""
    torch = torch_cuda
    rp, col, val = oracle.laplacian3d(*n_edge)
    n = len(rp) - 1
    if coding == "pairs":   # q-free iteration: x += alpha p rounded product by product
        monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
        monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
    else:                   # stored-q iteration (plain CSR / per-entry dictionaries): x = fma(alpha, p, x)
        monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "0")
        monkeypatch.setenv("SCHWZ_SPMV_PAIR", "0")
        monkeypatch.setenv("SCHWZ_SPMV_DICT", "0" if coding == "plain_csr" else "2")
    rng = np.random.default_rng(5)
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)
    A = schwz.Csr(rp, col, val)
    assert A.format() == {"pairs": 3, "plain_csr": 0, "dictionary": 1}[coding]
    cg = schwz.Pcg(A, 1)

    def solve(mode, iters, rtol):
        monkeypatch.setenv("SCHWZ_CG_DEFERX", mode)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, iters)
        return it, rn, d_x.cpu().numpy()

    for iters in (1, 2, 15, 16, 17, 31, 32, 33, 50):
        it0, rn0, x_plain = solve("0", iters, 0.0)
        assert cg.flavour() & 4 == 0
        it1, rn1, x_def = solve("2", iters, 0.0)
        assert cg.flavour() & 4 == 4
        assert it0 == it1 == iters and rn0 == rn1
        assert np.array_equal(x_plain, x_def), iters
    exp, it_o, rn_o = oracle.pcg(rp, col, val, b, x0, 1, 0.0, 33)
    assert np.abs(solve("2", 33, 0.0)[2] - exp).max() <= RTOL_CG * np.abs(exp).max()
    for rtol in (1e-3, 1e-6, 1e-10):
        it0, rn0, x_plain = solve("0", n, rtol)
        it1, rn1, x_def = solve("2", n, rtol)
        assert it0 == it1 and rn0 == rn1 and it0 < n
        assert np.array_equal(x_plain, x_def), rtol


def _slab_local_matrix(schwz, shape, P, me, overlap=2):
    """local_matrix of subdomain `me` of a z-slab partition: interior planes in natural order, the
    overlap planes appended at the end (rows next to them carry one far-away column); overlap = 4:
    three planes per side, appended layer by layer (lower 1, upper 1, lower 2, upper 2, ...)."""
    prob = schwz.Problem.laplacian(3, *shape)
    sd = schwz.Subdomain(prob, P, me, overlap, schwz.partition_regular(prob.N, P))
    return sd.local_matrix()


@pytest.mark.parametrize("case", [("cube", (256, 4, 12), "512"), ("cube", (256, 4, 10), "1024"), ("cube", (512, 4, 8), "512"),
                                  ("cube", (512, 4, 8), "1024"), ("cube", (256, 8, 7), "512"), ("slab", (256, 4, 30), "512"),
                                  ("slab", (256, 4, 30), "1024"), ("end", (256, 4, 24), "512"),
                                  ("slab4", (256, 4, 36), "512"), ("first", (256, 4, 24), "1024"),
                                  # x lines of 1024 entries: the fused launch takes bands of 2048 rows (two lines)
                                  ("cube", (1024, 4, 10), "1024"), ("slab", (1024, 4, 30), "1024")])
def test_z_sweep_update_launch_matches_the_gather_walk(schwz, oracle, torch_cuda, monkeypatch, case):
    """The z-sweep walk of the q-free update launch (a band of rows swept through consecutive planes,
    every operand of the canonical stencil layout read from an LDS ring of plane windows) against the
    chunk-by-chunk gather walk of the same launch: forced on small matrices (SCHWZ_SPMV_SWEEP=2), cubes
    with one / two / four bands and 512- or 1024-row bands, the local matrices of a middle and an end
    slab (appended overlap planes, boundary planes walked the generic way in the same launch), with
    the deferred x update the walk is built for (with the in-launch update the launch falls back to
    the gather walk: also run).  x lines of 256 and 512 entries: a chunk's pattern ids must run-length
    code for the walk.  Every row sees the same products in the same order, so one CG iteration is bit
    identical; later ones differ only through the order in which the per-workgroup partial sums of
    r.z are folded."""
    torch = torch_cuda
    kind, shape, T = case
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
    monkeypatch.setenv("SCHWZ_SPMV_SWEEP", "2")
    monkeypatch.setenv("SCHWZ_SWEEP_T", T)
    monkeypatch.setenv("SCHWZ_SWEEP_L", "4")
    if kind == "cube":
        rp, col, val = oracle.laplacian3d(*shape)
    elif kind == "slab4":
        rp, col, val = _slab_local_matrix(schwz, shape, 3, 1, overlap=4)
    else:
        rp, col, val = _slab_local_matrix(schwz, shape, 3, {"slab": 1, "end": 2, "first": 0}[kind])
    n = len(rp) - 1
    rng = np.random.default_rng(11)
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)
    A = schwz.Csr(rp, col, val)
    assert A.format() == 3 and A.symmetric() and A.sweep_slots() > 0
    # the appended overlap planes of a slab are chained to its interior: nothing is left to a companion launch
    assert A.sweep_left_out() == 0
    cg = schwz.Pcg(A, 1)

    def solve(sweep, defer, iters, rtol=0.0, start="0"):
        monkeypatch.setenv("SCHWZ_CG_SWEEP", sweep)
        monkeypatch.setenv("SCHWZ_CG_DEFERX", defer)
        monkeypatch.setenv("SCHWZ_CG_SWEEPSTART", start)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, iters)
        return it, rn, d_x.cpu().numpy()

    # the solve started in the walk as well (start residual in the INIT form of the update walk, p0 = D^-1 r0
    # and p0.(A p0) from the FIRST form of the fused launch): the same rows, but rho0 is folded from other
    # partial sums, so x agrees to rounding instead of bit for bit
    for iters in (1, 2, 7, 20):
        _, rn0, x_ref = solve("1", "2", iters)
        assert cg.flavour() & 32 == 0
        _, rn1, x_st = solve("1", "2", iters, start="1")
        assert cg.flavour() & 56 == 56, cg.flavour()
        assert np.abs(x_ref - x_st).max() <= 1e-12 * np.abs(x_ref).max(), iters
        assert abs(rn0 - rn1) <= 1e-10 * rn0
    it0, rn0, x_ref = solve("1", "2", n, 1e-9)
    it1, rn1, x_st = solve("1", "2", n, 1e-9, start="1")
    assert abs(it0 - it1) <= 1 and np.abs(x_ref - x_st).max() <= 1e-8 * np.abs(x_ref).max()
    # zero iterations: the start launch alone (residual norm), x untouched
    it0, rn0, x_ref = solve("1", "2", 0)
    it1, rn1, x_st = solve("1", "2", 0, start="1")
    assert it0 == it1 == 0 and abs(rn0 - rn1) <= 1e-13 * rn0 and np.array_equal(x_ref, x_st)

    for defer in ("0", "2"):
        it0, rn0, x_ref = solve("0", defer, 1)
        assert cg.flavour() & 24 == 0
        it1, rn1, x_sw = solve("1", defer, 1)
        # 16: the fused direction + p.(A p) launch walked in z-sweeps, 8: the update launch (deferred x only)
        assert cg.flavour() & 24 == (24 if defer == "2" else 16), cg.flavour()
        assert it0 == it1 == 1
        assert np.array_equal(x_ref, x_sw)
        assert abs(rn0 - rn1) <= 1e-14 * rn0
        for iters in (2, 7, 20):
            _, rn0, x_ref = solve("0", defer, iters)
            _, rn1, x_sw = solve("1", defer, iters)
            assert np.abs(x_ref - x_sw).max() <= 1e-12 * np.abs(x_ref).max(), (defer, iters)
            assert abs(rn0 - rn1) <= 1e-10 * rn0
    exp, _, _ = oracle.pcg(rp, col, val, b, x0, 1, 0.0, 20)
    assert np.abs(solve("1", "2", 20)[2] - exp).max() <= RTOL_CG * np.abs(exp).max()
    it0, _, x_ref = solve("0", "2", n, 1e-9)
    it1, _, x_sw = solve("1", "2", n, 1e-9)
    assert abs(it0 - it1) <= 1 and np.abs(x_ref - x_sw).max() <= 1e-8 * np.abs(x_ref).max()


@pytest.mark.parametrize("walk", [False, True])
def test_pcg_accepts_a_right_hand_side_that_is_only_8_byte_aligned(schwz, oracle, torch_cuda, monkeypatch, walk):
    """The CG start residual reads b with 16-byte loads; the caller's b need only be aligned like
    a double (x must be 16-byte aligned, which the entry point checks).  Chunk-by-chunk start launch and
    the start launch of the z-sweep walk (forced on a small grid)."""
    torch = torch_cuda
    if walk:
        for k, v in (("SCHWZ_SPMV_PATTERN", "2"), ("SCHWZ_SPMV_PAIR", "2"), ("SCHWZ_SPMV_SWEEP", "2"),
                     ("SCHWZ_SWEEP_T", "512"), ("SCHWZ_CG_DEFERX", "2")):
            monkeypatch.setenv(k, v)
    rp, col, val = oracle.laplacian3d(256, 4, 12) if walk else oracle.laplacian3d(24, 24, 24)
    n = len(rp) - 1
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n)
    A = schwz.Csr(rp, col, val)
    cg = schwz.Pcg(A, 1)
    res = []
    for shift in (0, 1):
        buf = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
        view = buf[shift:shift + n]
        view.copy_(torch.from_numpy(b))
        assert view.data_ptr() % 16 == 8 * shift
        d_x = torch.zeros(n, dtype=torch.float64, device="cuda")
        it, rn = cg.solve(view.data_ptr(), d_x.data_ptr(), 0.0, 20)
        res.append((d_x.cpu().numpy(), rn))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    assert (cg.flavour() & 32 != 0) == walk
    with pytest.raises(schwz.capi.SchwzError):
        d_x = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
        cg.solve(buf.data_ptr(), d_x[1:].data_ptr(), 0.0, 2)


@pytest.mark.parametrize("seed", range(12))
def test_pair_coding_on_random_banded_matrices(schwz, oracle, torch_cuda, monkeypatch, seed):
    """Random banded matrices (random sets of diagonals, some reaching almost across the whole
    matrix, piecewise constant values so that pair tables exist, rows near both ends losing the
    entries that fall outside): the row-pair SpMV against plain CSR bit for bit, and the q-free
    CG (symmetric and not quite symmetric values, i.e. with and without the upper-triangle
    tables) against the oracle.  Exercises the per-pattern decision between 16-byte gathers and
    the element-wise path at the ends of the vector."""
    import scipy.sparse as sp
    torch = torch_cuda
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(700, 6000))
    if seed % 3 == 0:
        n |= 1   # odd sizes: the last pair has one row
    nd = int(rng.integers(1, 5))
    offs = sorted(set(int(o) for o in np.concatenate([rng.integers(1, 40, nd), rng.integers(1, n - 1, 2)])))
    blocks = (np.arange(n) // 512) % 3
    diags, offsets = [], []
    for o in offs:
        v = -(0.2 + 0.1 * ((blocks[:n - o] + o) % 3))
        diags += [v, v]
        offsets += [o, -o]
    M = sp.diags(diags, offsets, shape=(n, n), format="csr")
    d = np.asarray(abs(M).sum(axis=1)).ravel() + 1.0 + 0.5 * blocks
    M = (M + sp.diags(d)).tocsr()
    M.sort_indices()
    symmetric = seed % 2 == 0
    val = M.data.copy()
    if not symmetric:
        val[int(M.indptr[n // 2]) + 0] *= 1.0 + 2.0 ** -30   # one entry off its mirror image
    rp, col = M.indptr.astype(np.int32), M.indices.astype(np.int32)
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
    monkeypatch.setenv("SCHWZ_DIAG_DICT", "0")
    A = schwz.Csr(rp, col, val)
    assert A.format() == 3
    assert col[M.indptr[n // 2]] != n // 2   # the perturbed entry is an off-diagonal one
    assert A.symmetric() == symmetric
    x = _dev(torch, rng.standard_normal(n))
    y0 = torch.zeros(n, dtype=torch.float64, device="cuda")
    y6 = torch.zeros(n, dtype=torch.float64, device="cuda")
    A.spmv(x.data_ptr(), y0.data_ptr(), 1.0, 0.0, 0)
    A.spmv(x.data_ptr(), y6.data_ptr(), 1.0, 0.0, 6)
    torch.cuda.synchronize()
    assert torch.equal(y0, y6)
    exp = oracle.spmv(rp, col, val, x.cpu().numpy())
    assert np.abs(y0.cpu().numpy() - exp).max() <= 1e-12 * max(np.abs(exp).max(), 1.0)
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)
    for mode in ("0", "2"):   # x updated inside the iteration / deferred
        monkeypatch.setenv("SCHWZ_CG_DEFERX", mode)
        cg = schwz.Pcg(A, 1)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 15)
        ex, it_o, rn_o = oracle.pcg(rp, col, val, b, x0, 1, 0.0, 15)
        assert it == it_o == 15
        assert np.abs(d_x.cpu().numpy() - ex).max() <= RTOL_CG * np.abs(ex).max()
        assert abs(rn - rn_o) <= 1e-8 * max(rn_o, 1e-300)


@pytest.mark.parametrize("kind", ["tridiagonal", "five_point_wide", "seven_point_with_extra_band"])
def test_canonical_stencil_layout_variants(schwz, oracle, torch_cuda, monkeypatch, kind):
    """Single-table matrices whose commonest row pair reads {.., -1, 0, +1, ..}: waves whose
    patterns all fit that layout take the offset-0 operands from the -1 and +1 gathers.  Layouts
    with filler slots (1-D: no outer offsets; 2-D: one each side) and a matrix in which some rows
    carry an entry outside the layout (those waves walk the generic table): SpMV bit for bit
    against plain CSR and against SCHWZ_SPMV_CANON=0, CG against the oracle."""
    import scipy.sparse as sp
    torch = torch_cuda
    rng = np.random.default_rng(17)
    if kind == "tridiagonal":
        n = 5001
        M = sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n), format="lil")
    elif kind == "five_point_wide":
        nx, ny = 300, 21
        n = nx * ny
        rp0, col0, val0 = oracle.laplacian2d(21)   # only for the generator's conventions
        ex = sp.diags([-1.0, -1.0], [-1, 1], shape=(nx, nx))
        ey = sp.diags([-1.0, -1.0], [-1, 1], shape=(ny, ny))
        M = (sp.kron(sp.identity(ny), ex) + sp.kron(ey, sp.identity(nx)) + 4.0 * sp.identity(n)).tolil()
    else:
        rp0, col0, val0 = oracle.laplacian3d(24, 20, 16)
        n = len(rp0) - 1
        M = sp.csr_matrix((val0, col0, rp0), shape=(n, n)).tolil()
        for i in range(1000, 1400, 7):      # a few rows with one more (symmetric) coupling far away
            j = i + 3000
            M[i, j] = -0.25
            M[j, i] = -0.25
            M[i, i] += 0.25
            M[j, j] += 0.25
    M = M.tocsr()
    M.sort_indices()
    rp, col, val = M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.copy()
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
    x = _dev(torch, rng.standard_normal(n))
    outs = []
    for canon in ("1", "0"):
        monkeypatch.setenv("SCHWZ_SPMV_CANON", canon)
        A = schwz.Csr(rp, col, val)
        assert A.format() == 3
        y0 = torch.zeros(n, dtype=torch.float64, device="cuda")
        y6 = torch.zeros(n, dtype=torch.float64, device="cuda")
        A.spmv(x.data_ptr(), y0.data_ptr(), 1.0, 0.0, 0)
        A.spmv(x.data_ptr(), y6.data_ptr(), 1.0, 0.0, 6)
        torch.cuda.synchronize()
        assert torch.equal(y0, y6)
        b = rng.standard_normal(n) if not outs else outs[0][2]
        cg = schwz.Pcg(A, 1)
        d_b, d_x = _dev(torch, b), torch.zeros(n, dtype=torch.float64, device="cuda")
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 12)
        outs.append((d_x.cpu().numpy(), rn, b))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    ex_x, it_o, rn_o = oracle.pcg(rp, col, val, outs[0][2], None, 1, 0.0, 12)
    assert np.abs(outs[0][0] - ex_x).max() <= RTOL_CG * np.abs(ex_x).max()


@pytest.mark.parametrize("vt", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("it", ["int32", "int64"])
def test_gather_scatter_every_reference_instantiation(schwz, torch_cuda, vt, it):
    _gather_scatter_typed(schwz, torch_cuda, vt, it, 5000, 7000)


@pytest.mark.parametrize("vt", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("it", ["int32", "int64"])
def test_gather_scatter_every_reference_instantiation_past_the_launch_cap(schwz, torch_cuda, vt, it):
    """n = 600 001 > 2048 * 256: the typed kernels run with a capped grid and stride."""
    _gather_scatter_typed(schwz, torch_cuda, vt, it, 600001, 700001)


def _gather_scatter_typed(schwz, torch_cuda, vt, it, n, m):
    """Gather / Scatter for the eight (value, index) type pairs the reference instantiates
    (gather_kernel.cu:112-146, scatter_kernel.cu:109-142) and its four ops, against numpy with the
    same element type (bit exact: one operation per element, integer avg = integer division)."""
    torch = torch_cuda
    rng = np.random.default_rng(7)
    vcode = {"float32": 0, "float64": 1, "int32": 2, "int64": 3}[vt]
    icode = {"int32": 0, "int64": 1}[it]
    idx = rng.permutation(m)[:n].astype(it)          # distinct targets: the scatter has no collisions
    src_g = (rng.standard_normal(m) * 100).astype(vt)
    src_s = (rng.standard_normal(n) * 100).astype(vt)
    d_idx = torch.from_numpy(idx).cuda()
    for op in (schwz.capi.OP_COPY, schwz.capi.OP_ADD, schwz.capi.OP_DIFF, schwz.capi.OP_AVG):
        def ref(into, frm):
            if op == schwz.capi.OP_COPY:
                return frm.copy()
            if op == schwz.capi.OP_ADD:
                return frm + into
            if op == schwz.capi.OP_DIFF:
                return frm - into
            s = frm + into
            if vt.startswith("float"):
                return (s / np.array(2, dtype=vt)).astype(vt)
            return (np.sign(s) * (np.abs(s) // 2)).astype(vt)  # C++ integer division truncates toward zero
        into0 = (rng.standard_normal(n) * 10).astype(vt)
        d_from, d_into = torch.from_numpy(src_g).cuda(), torch.from_numpy(into0.copy()).cuda()
        schwz.capi.check(schwz.capi.lib.schwz_gather_typed(n, d_idx.data_ptr(), icode, d_from.data_ptr(),
                                                           d_into.data_ptr(), vcode, op, None))
        torch.cuda.synchronize()
        assert np.array_equal(d_into.cpu().numpy(), ref(into0, src_g[idx]))
        big0 = (rng.standard_normal(m) * 10).astype(vt)
        d_from, d_big = torch.from_numpy(src_s).cuda(), torch.from_numpy(big0.copy()).cuda()
        schwz.capi.check(schwz.capi.lib.schwz_scatter_typed(n, d_idx.data_ptr(), icode, d_from.data_ptr(),
                                                            d_big.data_ptr(), vcode, op, None))
        torch.cuda.synchronize()
        exp = big0.copy()
        exp[idx] = ref(big0[idx], src_s)
        assert np.array_equal(d_big.cpu().numpy(), exp)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SCHWZ_FUZZ_SEEDS", "10"))))  # more seeds: a fuzz run
def test_z_sweep_walk_on_random_grid_shapes(schwz, oracle, torch_cuda, monkeypatch, seed):
    """Random grid shapes and slab cuts through the z-sweep walk (forced on small matrices): x lines of 256 /
    512 / 1024 entries, 4-8 lines per plane, cubes and first / middle / last slabs of 2-4 with overlap 2 or 4.
    Wherever the upload builds the walk, one CG iteration (start launch chunk by chunk) is bit-identical to
    the gather walk, the solve that starts in the walk agrees to rounding, and 12 iterations match the oracle."""
    torch = torch_cuda
    rng = np.random.default_rng(1000 + seed)
    nx = int(rng.choice([256, 256, 512, 1024]))
    ny = int(rng.choice({256: [4, 6, 8], 512: [4, 5, 6], 1024: [4, 5]}[nx]))  # whole chunks of 512 rows per plane
    _walk_fuzz_case(schwz, oracle, torch, monkeypatch, rng, nx, ny)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SCHWZ_FUZZ_SEEDS", "10"))))
def test_z_sweep_walk_on_planes_that_are_not_whole_chunks(schwz, oracle, torch_cuda, monkeypatch, seed):
    """The same walk on planes whose size is not a multiple of the 512-row chunk (x lines of 96 ... 600 entries,
    e.g. 200 x 9): the bands of a plane no longer coincide with the chunks, pattern ids are read as bytes, the
    last band of every plane is partial (round 3, CsrView::sweep_gen_mode).  Same checks: bit identity of one CG
    iteration with the chunk-by-chunk kernels, the solve that starts in the walk, 12 iterations against the
    oracle; cubes and slabs with overlap."""
    torch = torch_cuda
    rng = np.random.default_rng(5000 + seed)
    while True:
        nx = int(rng.choice([96, 120, 200, 250, 300, 320, 384, 600]))
        ny = int(rng.integers(3, 12))
        if (nx * ny) % 512 != 0 and nx * ny >= 1024:
            break
    _walk_fuzz_case(schwz, oracle, torch, monkeypatch, rng, nx, ny, expect_gen=True)


@pytest.mark.parametrize("case", [(512, 1, 0), (1024, 1, 0), (640, 1, 0), (512, 3, 1), (768, 2, 0), (1000, 2, 1)])
def test_z_sweep_walk_on_two_dimensional_grids(schwz, oracle, torch_cuda, monkeypatch, case):
    """The 5-point (2-D) Laplacian of the reference's own generator (initialization.cpp:214-265) through the same walk:
    the x line plays the plane, the +-N neighbours sit in the previous / next line's window, the halo around a band
    is its left and right neighbour (round 3).  Whole grids and row-block subdomains with overlap, line lengths that
    are whole chunks and not (640, 1000: byte ids, partial last band): bit identity of one CG iteration with the
    chunk-by-chunk kernels, the solve that starts in the walk, 12 iterations against the oracle."""
    torch = torch_cuda
    n1d, P, me = case
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
    monkeypatch.setenv("SCHWZ_SPMV_SWEEP", "2")
    prob = schwz.Problem.laplacian(2, n1d)
    sd = schwz.Subdomain(prob, P, me, 2, schwz.partition_regular(prob.N, P))
    rp, col, val = sd.local_matrix()
    rng = np.random.default_rng(77 + n1d + P)
    _walk_checks(schwz, oracle, torch, monkeypatch, rng, rp, col, val, must_walk=True, tag=case)


def _walk_fuzz_case(schwz, oracle, torch, monkeypatch, rng, nx, ny, expect_gen=False):
    nz = int(rng.integers(9, 30))
    P = int(rng.integers(1, 5))
    me = int(rng.integers(0, P))
    overlap = int(rng.choice([2, 2, 4]))
    monkeypatch.setenv("SCHWZ_SPMV_PATTERN", "2")
    monkeypatch.setenv("SCHWZ_SPMV_PAIR", "2")
    monkeypatch.setenv("SCHWZ_SPMV_SWEEP", "2")
    if P == 1:
        rp, col, val = oracle.laplacian3d(nx, ny, nz)
    else:
        rp, col, val = _slab_local_matrix(schwz, (nx, ny, nz * P), P, me, overlap=overlap)
    # three lines per plane: two thirds of the rows sit on a y face, the commonest row pattern lacks a +-NX entry and the
    # matrix gets no canonical 7-slot layout (spmv_pair.hip, "canonical stencil layout") -- the chunk kernels serve it
    _walk_checks(schwz, oracle, torch, monkeypatch, rng, rp, col, val, must_walk=expect_gen and P == 1 and ny >= 4,
                 tag=(nx, ny, nz, P, me, overlap))


def _walk_checks(schwz, oracle, torch, monkeypatch, rng, rp, col, val, must_walk, tag):
    n = len(rp) - 1
    A = schwz.Csr(rp, col, val)
    assert A.format() == 3
    if A.sweep_slots() == 0:
        assert not must_walk, "this matrix must walk: %r" % (tag,)
        pytest.skip("no walk for %r" % (tag,))
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)
    cg = schwz.Pcg(A, 1)

    def solve(sweep, iters, start="0", rtol=0.0):
        monkeypatch.setenv("SCHWZ_CG_SWEEP", sweep)
        monkeypatch.setenv("SCHWZ_CG_DEFERX", "2")
        monkeypatch.setenv("SCHWZ_CG_SWEEPSTART", start)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, iters)
        return (rn, it) if rtol > 0.0 else rn, d_x.cpu().numpy()

    rn0, x_ref = solve("0", 1)
    rn1, x_sw = solve("1", 1)
    assert cg.flavour() & 8 == 8, (cg.flavour(), tag)
    assert np.array_equal(x_ref, x_sw), tag
    rn2, x_st = solve("1", 1, start="1")
    assert np.abs(x_ref - x_st).max() <= 1e-13 * np.abs(x_ref).max()
    exp, _, _ = oracle.pcg(rp, col, val, b, x0, 1, 0.0, 12)
    assert np.abs(solve("1", 12, start="1")[1] - exp).max() <= RTOL_CG * np.abs(exp).max()
    # the virtual first direction (p0 = D^-1 r0 never stored: rebuilt from r0 by its three readers, round 3) against
    # the stored one: the same bits, also past the 16 slots of the direction ring (direction 16 lands on the r0 buffer)
    for iters in (12, 19):
        monkeypatch.setenv("SCHWZ_CG_P0VIRTUAL", "0")
        rn_s, x_s = solve("1", iters, start="1")
        assert cg.flavour() & 64 == 0
        in_walk = cg.flavour() & 32 == 32  # the solve started in the walk (no rows left to the chunk launches)
        monkeypatch.setenv("SCHWZ_CG_P0VIRTUAL", "1")
        rn_v, x_v = solve("1", iters, start="1")
        assert (cg.flavour() & 64 == 64) == in_walk, (cg.flavour(), tag)
        assert np.array_equal(x_s, x_v) and rn_s == rn_v, (tag, iters)
    # the last direction of a fixed-work solve is never stored either (rebuilt inside the x update; and, because this
    # test asks for the residual norm, rebuilt in memory for the postponed last update launch)
    for iters in (2, 10, 17):
        monkeypatch.setenv("SCHWZ_CG_PLASTVIRTUAL", "0")
        rn_s, x_s = solve("1", iters, start="1")
        assert cg.flavour() & 128 == 0
        in_walk = cg.flavour() & 32 == 32
        monkeypatch.setenv("SCHWZ_CG_PLASTVIRTUAL", "1")
        rn_v, x_v = solve("1", iters, start="1")
        assert (cg.flavour() & 128 == 128) == in_walk, (cg.flavour(), tag)
        assert np.array_equal(x_s, x_v) and rn_s == rn_v, (tag, iters)
    monkeypatch.delenv("SCHWZ_CG_PLASTVIRTUAL")
    # ... and a solve to a tolerance (the host polls the state, the x update takes the iterations carried out)
    monkeypatch.setenv("SCHWZ_CG_P0VIRTUAL", "0")
    st_s, x_s = solve("1", 300, start="1", rtol=1e-3)
    monkeypatch.setenv("SCHWZ_CG_P0VIRTUAL", "1")
    st_v, x_v = solve("1", 300, start="1", rtol=1e-3)
    assert np.array_equal(x_s, x_v) and st_s == st_v and st_s[1] > 1, (tag, st_s, st_v)
    monkeypatch.delenv("SCHWZ_CG_P0VIRTUAL")
