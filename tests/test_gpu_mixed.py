"""The mixed-precision local solve on the GPU (schwz_pcg_f32, Metadata.local_solver_precision = "single"): fp32 CG
on the fp64 start residual, the correction added in fp64.  The product q = A32 p against a longdouble row sum with
the derived rounding bound, whole solves against the correction-form restatement in longdouble with a tolerance
sized by the same text run in float32, the edge cases, whole RAS runs in both precisions, and the C++ mirror.

Matrices: the smallest at which the kernels can go wrong -- more than one 256-row tile, a partial last tile,
n % 4 != 0 (ani4_crop, rand777, band1501), rows of 3..9 entries (ani4_crop: the 16-entry form of the stream
kernel), rows of 25 entries (band1501: its 32-entry form), and a matrix with one row of 40 entries and one
diagonal-only row, which takes the fallback SpMV kernel (rows beyond 32 entries).

Size-dependent branches of csrc/cg_f32.hip (pcg_f32_build), each crossed by a Laplacian of its own in
test_large_grids_*: (1) the vector launches give every lane one quad up to 4 * 256 * kMaxGrid = 2 097 152 entries
and stride beyond; (2) the stream kernel runs short-lived workgroups of 3 consecutive tiles while that grid fits
kMaxGrid = 2048 workgroups (6144 tiles, about 1.57 M rows) and persistent workgroups beyond; (3) on planes of more
than 2048 tiles the tile sequence of an XCD is the explicit one of CsrView::stream_order.  130^3 (2 197 000 rows, 8583
tiles) crosses (1) and (2); 1024 x 1024 x 4 crosses all three.  In both the consumers fold 2048 partial sums per bank.
"""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hp_reference as hp
from hp_reference import LD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
MPIEXEC = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
DRIVER = os.path.join(ROOT, "schwarz-lib_amd", "build", "mixed_driver")
U32 = 2.0 ** -24   # unit roundoff of float32
NAMES = ["lap3d_16x10x7", "lap3d_12x12x12", "ani4_crop", "rand777", "band1501"]


def _band1501():
    """Seeded SPD band matrix of 1501 rows, 12 entries either side of the diagonal (rows of 13..25 entries: the
    32-entry form of the stream kernel, 19 tiles), off-diagonals negative, weakly diagonally dominant."""
    import scipy.sparse as sp
    rng = np.random.default_rng(1501)
    n = 1501
    offs = list(range(1, 13))
    a = sp.diags([rng.uniform(-1.0, -0.1, n - k) for k in offs], offs, shape=(n, n), format="csr")
    a = a + a.T
    d = np.asarray(abs(a).sum(axis=1)).ravel() + rng.uniform(0.01, 0.02, size=n)   # weakly dominant: 40 updates stay short of convergence
    a = (a + sp.diags(d)).tocsr()
    a.sort_indices()
    assert np.diff(a.indptr).max() == 25
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def _rand777():
    """Seeded SPD matrix of 777 rows, diagonally dominant: about 5 entries per row, row 100 with 40 entries (its
    columns get the mirrored entry), row 200 diagonal only."""
    import scipy.sparse as sp
    rng = np.random.default_rng(777)
    n = 777
    a = sp.random(n, n, density=2.0 / n, random_state=np.random.RandomState(777), format="lil")
    a[200, :] = 0
    a[:, 200] = 0
    a[100, :] = 0
    a[:, 100] = 0
    others = rng.choice(np.setdiff1d(np.arange(n), [100, 200]), size=39, replace=False)
    a[100, others] = rng.uniform(-1.0, 1.0, size=39)
    a = a.tocsr()
    a = a + a.T
    a.setdiag(0)
    a.eliminate_zeros()
    d = np.asarray(abs(a).sum(axis=1)).ravel() + rng.uniform(1.0, 2.0, size=n)
    a = (a + sp.diags(d)).tocsr()
    a.sort_indices()
    ln = np.diff(a.indptr)
    assert ln[100] == 40 and ln[200] == 1 and ln.max() == 40
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _matrix(name):
    import oracle as O
    O.build()
    if name.startswith("lap3d_"):
        return O.laplacian3d(*(int(k) for k in name[6:].split("x")))
    if name == "ani4_crop":
        g = np.load(os.path.join(G, "ani4_crop.npz"))
        return g["rp"].astype(np.int32), g["col"].astype(np.int32), g["val"].astype(np.float64)
    if name == "band1501":
        return _band1501()
    assert name == "rand777"
    return _rand777()


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(b, x0) of a matrix: seeded, shared by the tests."""
    n = len(_matrix(name)[0]) - 1
    rng = np.random.default_rng(len(name) + n)
    return rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)


def _precond(name, precond, dtype, record=None):
    rp, col, val = _matrix(name)
    M = hp.precond_jacobi(rp, col, val, dtype) if precond else hp.precond_none(dtype)
    if record is None:
        return M

    def apply(v):
        record["r"] = np.array(v, dtype=dtype)   # the recurred residual the solve last applied M to
        return M(v)
    return apply


@functools.lru_cache(maxsize=None)
def _start(name):
    """(r0 / nu in longdouble, nu) of the shared problem."""
    hp.require_extended_precision()
    rp, col, val = _matrix(name)
    b, x0 = _problem(name)
    r0 = np.asarray(b, dtype=LD) - hp.spmv(rp, col, val, x0, LD)
    nu = np.sqrt(hp.dot(r0, r0))
    return r0 / nu, nu


KS = (1, 10, 40)


@functools.lru_cache(maxsize=None)
def _fixed_reference(name, precond):
    """x after k in KS updates of the correction-form solve, in longdouble and in float32 (the same text)."""
    rp, col, val = _matrix(name)
    _, x0 = _problem(name)
    rhat, nu = _start(name)
    out = {}
    for dtype in (LD, np.float32):
        keep = {k: None for k in KS}
        hp.pcg(rp, col, val, rhat.astype(dtype), None, _precond(name, precond, dtype), max(KS), 0.0, dtype, keep)
        out[dtype] = {k: np.asarray(x0, dtype=LD) + nu * np.asarray(keep[k], dtype=LD) for k in KS}
    return out


def _dev(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype or torch.float64)


@pytest.fixture(scope="module")
def solvers(schwz, torch_cuda):
    made = {}

    def get(name, precond):
        if (name, precond) not in made:
            csr = made.get(name) or schwz.Csr(*_matrix(name))
            made[name] = csr
            made[(name, precond)] = schwz.PcgF32(csr, precond)
        return made[(name, precond)]
    yield get
    made.clear()


# ---- 1. the product ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_spmv_meets_the_rowwise_fp32_bound(schwz, torch_cuda, solvers, name):
    """|q_i - q^_i| <= gamma_k sum_j |a32_ij| |p32_j|, k = row length + 1, u = 2^-24 (Higham, Accuracy and Stability,
    eq. 3.5: k - 1 additions and one product per term, summed in any order), against the longdouble row sums of the
    fp32-rounded values and vector.  p.q is a sum of exact products added up in float64: gamma_n of 2^-53."""
    hp.require_extended_precision()
    torch = torch_cuda
    rp, col, val = _matrix(name)
    n = len(rp) - 1
    a32 = val.astype(np.float32)
    p32 = np.random.default_rng(5).uniform(-1.0, 1.0, n).astype(np.float32)
    s = solvers(name, schwz.capi.PRECOND_NONE)
    d_p, d_q = _dev(torch, p32, torch.float32), torch.full((n,), float("nan"), device="cuda", dtype=torch.float32)
    pq = s.spmv(d_p.data_ptr(), d_q.data_ptr())
    q = d_q.cpu().numpy()
    ref = hp.spmv(rp, col, a32, p32, LD)
    mag = hp.spmv(rp, col, np.abs(a32), np.abs(p32), LD)
    k = (np.diff(rp) + 1).astype(LD)
    gamma = k * LD(U32) / (1 - k * LD(U32))
    err = np.abs(q.astype(LD) - ref)
    assert np.all(np.isfinite(q))
    worst = int(np.argmax(err - gamma * mag))
    assert np.all(err <= gamma * mag), (worst, float(err[worst]), float((gamma * mag)[worst]))
    terms = p32.astype(LD) * q.astype(LD)
    gn = LD(n) * LD(hp.U64) / (1 - LD(n) * LD(hp.U64))
    assert abs(LD(pq) - terms.sum()) <= gn * np.abs(terms).sum(), (pq, float(terms.sum()))


@pytest.mark.parametrize("shape", [(130, 130, 130), (1024, 1024, 4)])
def test_large_grids_spmv(schwz, oracle, torch_cuda, shape):
    """The product and p.q past the size-dependent branches named at the top of this file (persistent workgroups
    of the stream kernel, the explicit XCD tile sequence, 2048 partial sums per bank): the same row-wise bound.
    The values 6 and -1 are exact in float32; the longdouble reference is the slicing stencil."""
    hp.require_extended_precision()
    torch = torch_cuda
    rp, col, val = oracle.laplacian3d(*shape)
    n = len(rp) - 1
    csr = schwz.Csr(rp, col, val)
    s = schwz.PcgF32(csr, schwz.capi.PRECOND_NONE)
    p32 = np.random.default_rng(11).uniform(-1.0, 1.0, n).astype(np.float32)
    d_p, d_q = _dev(torch, p32, torch.float32), torch.full((n,), float("nan"), device="cuda", dtype=torch.float32)
    pq = s.spmv(d_p.data_ptr(), d_q.data_ptr())
    pq2 = s.spmv(d_p.data_ptr(), d_q.data_ptr())
    q = d_q.cpu().numpy()
    ref = hp.stencil_apply(p32, shape, LD)
    ap = np.abs(p32)
    mag = 12 * ap.astype(LD) - hp.stencil_apply(ap, shape, LD)      # sum_j |a_ij| |p_j| = 6 |p_i| + the neighbours'
    k = (np.diff(rp) + 1).astype(LD)
    gamma = k * LD(U32) / (1 - k * LD(U32))
    err = np.abs(q.astype(LD) - ref)
    assert np.all(np.isfinite(q))
    worst = int(np.argmax(err - gamma * mag))
    assert np.all(err <= gamma * mag), (worst, float(err[worst]), float((gamma * mag)[worst]))
    terms = p32.astype(LD) * q.astype(LD)
    gn = LD(n) * LD(hp.U64) / (1 - LD(n) * LD(hp.U64))
    assert abs(LD(pq) - terms.sum()) <= gn * np.abs(terms).sum(), (pq, float(terms.sum()))
    assert pq == pq2
    s.close()
    csr.close()


def test_large_grids_solve_against_the_fp64_cg(schwz, oracle, torch_cuda):
    """130^3, 10 Jacobi iterations from a random x0, past branches (1) and (2): against the fp64 CG of the library
    (whose own error is nine digits below), ||x_single - x_double|| <= 8 x what the float32 restatement of the
    correction form (slicing stencil) differs from it by; two runs give the same bits."""
    torch = torch_cuda
    shape = (130, 130, 130)
    rp, col, val = oracle.laplacian3d(*shape)
    n = len(rp) - 1
    rng = np.random.default_rng(130)
    b, x0 = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    csr = schwz.Csr(rp, col, val)
    d_b = _dev(torch, b)
    d_x = _dev(torch, x0)
    its, _ = schwz.Pcg(csr, schwz.capi.PRECOND_JACOBI).solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 10)
    assert its == 10
    x64 = d_x.cpu().numpy()
    s = schwz.PcgF32(csr, schwz.capi.PRECOND_JACOBI)
    outs = []
    for _ in range(2):
        d_x = _dev(torch, x0)
        its, rn = s.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 10)
        assert its == 10 and np.isfinite(rn)
        outs.append(d_x.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))
    r0 = b - hp.stencil_apply(x0, shape, np.float64)
    nu = np.sqrt(hp.dot(r0, r0))
    f32 = np.float32
    e32, _ = hp.pcg(lambda v: hp.stencil_apply(v, shape, f32), None, None, (r0 / nu).astype(f32), None,
                    lambda v: np.asarray(v, dtype=f32) / f32(6), 10, 0.0, f32)
    delta_ref = float(np.linalg.norm(x0 + nu * e32.astype(np.float64) - x64))
    err = float(np.linalg.norm(outs[0] - x64))
    print("130^3: |x_single - x_double| = %.3e, delta_ref = %.3e" % (err, delta_ref))
    assert err <= 8 * delta_ref, (err, delta_ref)
    s.close()
    csr.close()


# ---- 2. fixed-work solves ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_fixed_work_solve_within_8x_of_what_fp32_rounding_does(schwz, torch_cuda, solvers, name, precond, k):
    """rtol = 0, exactly k updates from a random x0: ||x_gpu - x_LD|| <= 8 ||x_f32 - x_LD||, the restatement in
    float32 showing what fp32 rounding alone does; 8 covers another summation order (fp64-accumulated dots, 1/diag
    rounded once), as in the GMRES tests."""
    torch = torch_cuda
    b, x0 = _problem(name)
    ref = _fixed_reference(name, precond)
    x_ld, x_32 = ref[LD][k], ref[np.float32][k]
    delta_ref = float(np.linalg.norm((x_32 - x_ld).astype(np.float64)))
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    its, rn = solvers(name, precond).solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, k)
    x = d_x.cpu().numpy()
    err = float(np.linalg.norm((x.astype(LD) - x_ld).astype(np.float64)))
    print("%s precond %d k %d: |x_gpu - x_LD| = %.3e, delta_ref = %.3e" % (name, precond, k, err, delta_ref))
    assert its == k
    assert np.all(np.isfinite(x)) and np.isfinite(rn)
    assert err <= 8 * delta_ref, "error %.3e, delta_ref %.3e" % (err, delta_ref)


# ---- 3. tolerance solves ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_tolerance_solve_counts_and_true_residual(schwz, torch_cuda, solvers, name, precond):
    """rtol = 1e-4: the count within one of the float32 restatement's; the float64 true residual of the returned x is
    the recurred residual (<= rtol nu at the stop) plus the drift between true and recurred residual, which is
    rounding: <= 8 x the restatement's drift."""
    torch = torch_cuda
    rtol = 1e-4
    rp, col, val = _matrix(name)
    n = len(rp) - 1
    b, x0 = _problem(name)
    rhat, nu = _start(name)
    rec = {}
    e32, hist = hp.pcg(rp, col, val, rhat.astype(np.float32), None, _precond(name, precond, np.float32, rec), n, rtol,
                       np.float32)
    its_ref = len(hist) - 1
    assert 0 < its_ref < n
    true32 = rhat - hp.spmv(rp, col, val, np.asarray(e32, dtype=LD), LD)
    gap = float(nu * np.sqrt(hp.dot(true32 - rec["r"].astype(LD), true32 - rec["r"].astype(LD))))
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    its, rn = solvers(name, precond).solve(d_b.data_ptr(), d_x.data_ptr(), rtol, n)
    x = d_x.cpu().numpy()
    r = np.asarray(b, dtype=LD) - hp.spmv(rp, col, val, x, LD)
    res = float(np.sqrt(hp.dot(r, r)))
    print("%s precond %d: its %d (restatement %d), |b - A x| = %.3e, rtol nu = %.3e, gap = %.3e, reported %.3e"
          % (name, precond, its, its_ref, res, rtol * float(nu), gap, rn))
    assert abs(its - its_ref) <= 1, (its, its_ref)
    assert rn <= rtol * float(nu) * (1 + 1e-12)
    assert res <= rtol * float(nu) + 8 * gap, (res, rtol * float(nu), gap)


# ---- 4. edge cases ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lap3d_16x10x7", "rand777"])
def test_zero_start_residual_leaves_x_alone(schwz, torch_cuda, solvers, name):
    torch = torch_cuda
    n = len(_matrix(name)[0]) - 1
    d_b = torch.zeros(n, device="cuda", dtype=torch.float64)
    d_x = torch.zeros(n, device="cuda", dtype=torch.float64)
    d_x[1] = -0.0
    before = d_x.cpu().numpy().view(np.int64).copy()
    its, rn = solvers(name, schwz.capi.PRECOND_JACOBI).solve(d_b.data_ptr(), d_x.data_ptr(), 1e-6, 50)
    assert its == 0 and rn == 0.0
    assert np.array_equal(d_x.cpu().numpy().view(np.int64), before)


@pytest.mark.parametrize("name", ["lap3d_16x10x7", "rand777"])
def test_max_iters_zero_leaves_x_alone(schwz, torch_cuda, solvers, name):
    torch = torch_cuda
    b, x0 = _problem(name)
    d_b, d_x = _dev(torch, b), _dev(torch, x0)
    its, rn = solvers(name, schwz.capi.PRECOND_NONE).solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 0)
    assert its == 0
    assert np.array_equal(d_x.cpu().numpy().view(np.int64), x0.view(np.int64))
    nu = float(_start(name)[1])
    assert abs(rn - nu) <= 1e-6 * nu   # nu x the norm of the fp32-rounded unit residual


@pytest.mark.parametrize("name", NAMES)
def test_two_identical_solves_give_identical_bits(schwz, torch_cuda, solvers, name):
    torch = torch_cuda
    b, x0 = _problem(name)
    outs = []
    for _ in range(2):
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        its, rn = solvers(name, schwz.capi.PRECOND_JACOBI).solve(d_b.data_ptr(), d_x.data_ptr(), 1e-5, 200)
        outs.append((its, rn, d_x.cpu().numpy().view(np.int64).copy()))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][2], outs[1][2])


def test_value_beyond_fp32_is_refused_at_creation(schwz, torch_cuda):
    rp = np.array([0, 2, 4, 5], np.int32)
    col = np.array([0, 1, 0, 1, 2], np.int32)
    val = np.array([2.0, -1.0, -1.0, 1e300, 1.0])
    csr = schwz.Csr(rp, col, val)
    with pytest.raises(schwz.NotImplementedSchwz) as e:
        schwz.PcgF32(csr, schwz.capi.PRECOND_NONE)
    assert "(1, 1)" in str(e.value)
    # an infinity that is one already is no rounding overflow; a value fp32 holds is fine
    schwz.PcgF32(schwz.Csr(rp, col, np.array([2.0, -1.0, -1.0, 3e38, 1.0])), schwz.capi.PRECOND_JACOBI)


def test_other_preconditioners_are_refused(schwz, torch_cuda, solvers):
    csr = solvers("lap3d_16x10x7", 0).csr
    for code in (schwz.capi.PRECOND_BLOCK_JACOBI, schwz.capi.PRECOND_ILU, schwz.capi.PRECOND_ISAI):
        with pytest.raises(schwz.NotImplementedSchwz):
            schwz.PcgF32(csr, code)


# ---- 5.-8. whole RAS runs ---------------------------------------------------------------------------------------

def _run(schwz, P, settings_kw, metadata_kw):
    s = schwz.Settings(**settings_kw)
    m = schwz.Metadata(num_subdomains=P, **metadata_kw)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    return solver, m, solver.run()


def _lambda_min(shape):
    return sum(4.0 * np.sin(np.pi / (2 * (k + 1))) ** 2 for k in shape)


def _csr(rp, col, val):
    import scipy.sparse as sp
    n = len(rp) - 1
    return sp.csr_matrix((val, col, rp), shape=(n, n))


@pytest.mark.parametrize("shape, P, local_tol, iters_cpu", [
    ((12, 12, 12), 1, 0.0, 12), ((12, 12, 12), 3, 0.0, 22), ((16, 10, 7), 2, 0.0, 15), ((12, 12, 12), 3, 1e-4, None)])
def test_ras_single_follows_double(schwz, oracle, torch_cuda, shape, P, local_tol, iters_cpu):
    """Both precisions converge within one outer iteration of each other, to solutions whose float64 residuals
    meet the rule of test_ras_with_parilu_options and which differ by no more than the two residuals allow.
    iters_cpu: what a numpy restatement of an ADDITIVE Schwarz iteration took on the fixed-work cases, the same in
    both precisions (printed beside the counts of the library's restricted iteration, not asserted)."""
    tol = 1e-10
    A = _csr(*oracle.laplacian3d(*shape))
    N = A.shape[0]
    runs = {}
    for prec in ("double", "single"):
        solver, m, out = _run(schwz, P, dict(laplacian_dim=3, laplacian_shape=shape),
                              dict(tolerance=tol, max_iters=100, local_precond="block-jacobi", precond_max_block_size=1,
                                   local_solver_tolerance=local_tol, local_max_iters=10 if local_tol == 0.0 else -1,
                                   local_solver_precision=prec))
        x = np.asarray(out["solution"])
        runs[prec] = (out, x, float(np.linalg.norm(np.ones(N) - A @ x)))
        want = schwz.capi.PRECISION_F32 if prec == "single" else schwz.capi.PRECISION_F64
        for sd in solver.subdomains.values():
            assert sd.local_precision() == want
            if prec == "single":
                assert sd.cg_flavour() == 0 and sd.y_form() == 0 and not sd.early_pack_ok()
    (out_d, x_d, res_d), (out_s, x_s, res_s) = runs["double"], runs["single"]
    print("%s P %d local_tol %g: outer double %d single %d (numpy restatement %s), residuals %.3e %.3e"
          % (shape, P, local_tol, out_d["iter_count"], out_s["iter_count"], iters_cpu, res_d, res_s))
    assert out_d["converged"] and out_s["converged"]
    assert abs(out_s["iter_count"] - out_d["iter_count"]) <= 1
    assert res_d <= 10 * tol * np.sqrt(N) and res_s <= 10 * tol * np.sqrt(N), (res_d, res_s)
    assert np.linalg.norm(x_s - x_d) <= (res_s + res_d) / _lambda_min(shape)


def _write_mtx(tmp_path, rp, col, val):
    n = len(rp) - 1
    path = str(tmp_path / "a.mtx")
    rows = np.repeat(np.arange(n), np.diff(rp))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, rp[-1]))
        for r, c, v in zip(rows, col, val):
            f.write("%d %d %.17g\n" % (r + 1, c + 1, v))
    return path


def test_ras_general_matrix_single_follows_double(schwz, torch_cuda, tmp_path):
    rp, col, val = _matrix("ani4_crop")
    A = _csr(rp, col, val)
    N = A.shape[0]
    path = _write_mtx(tmp_path, rp, col, val)
    kw = dict(tolerance=1e-9, local_precond="block-jacobi", precond_max_block_size=1, local_solver_tolerance=1e-6)
    sk = dict(matrix_filename=path, explicit_laplacian=False)
    _, _, out_d = _run(schwz, 2, sk, dict(kw, max_iters=3000))
    assert out_d["converged"]
    solver, _, out_s = _run(schwz, 2, sk, dict(kw, max_iters=out_d["iter_count"] + 2, local_solver_precision="single"))
    res_d = float(np.linalg.norm(np.ones(N) - A @ np.asarray(out_d["solution"])))
    res_s = float(np.linalg.norm(np.ones(N) - A @ np.asarray(out_s["solution"])))
    print("ani4_crop P 2: outer double %d single %d, residuals %.3e %.3e"
          % (out_d["iter_count"], out_s["iter_count"], res_d, res_s))
    assert out_s["converged"]
    assert abs(out_s["iter_count"] - out_d["iter_count"]) <= 1
    assert res_s <= 10 * res_d, (res_s, res_d)
    assert all(sd.local_precision() == schwz.capi.PRECISION_F32 for sd in solver.subdomains.values())


@pytest.mark.parametrize("P", [1, 2])
def test_default_precision_changes_nothing(schwz, torch_cuda, P):
    kw = dict(tolerance=1e-9, max_iters=100, local_precond="block-jacobi", precond_max_block_size=1,
              local_solver_tolerance=0.0, local_max_iters=10)
    sk = dict(laplacian_dim=3, laplacian_shape=(16, 10, 7))
    s0, _, out0 = _run(schwz, P, sk, kw)
    s1, _, out1 = _run(schwz, P, sk, dict(kw, local_solver_precision="double"))
    assert out0["iter_count"] == out1["iter_count"]
    assert np.array_equal(np.asarray(out0["solution"]), np.asarray(out1["solution"]))
    for me in s0.subdomains:
        assert s0.subdomains[me].cg_flavour() == s1.subdomains[me].cg_flavour()
        assert s0.subdomains[me].y_form() == s1.subdomains[me].y_form()
        assert s1.subdomains[me].local_precision() == schwz.capi.PRECISION_F64


def test_switching_back_restores_the_fp64_path(schwz, torch_cuda, monkeypatch):
    """F32, one solve, F64, the next solve: the fp64 CG runs again, in the form it ran in before.  With
    SCHWZ_CG_DEFERX=2 (read per solve) the fp64 CG of this small subdomain defers x -- a flavour other than 0 -- and
    keeps y inside the x~ buffers, so the switch also goes from the unified form to a y of its own and back."""
    torch = torch_cuda
    monkeypatch.setenv("SCHWZ_CG_DEFERX", "2")
    kw = dict(tolerance=1e-9, max_iters=100, local_precond="block-jacobi", precond_max_block_size=1,
              local_solver_tolerance=0.0, local_max_iters=10)
    solver, m, out = _run(schwz, 1, dict(laplacian_dim=3, laplacian_shape=(12, 12, 12)), kw)
    sd = solver.subdomains[0]
    flavour, y_form = sd.cg_flavour(), sd.y_form()
    assert flavour != 0 and y_form != 0
    sd.set_local_precision(schwz.capi.PRECISION_F32)
    assert sd.local_precision() == schwz.capi.PRECISION_F32 and sd.y_form() == 0
    assert sd.algorithmic_bytes(1) < sd.algorithmic_bytes(0) + 136 * sd.local_size_x
    sd.local_solve()
    torch.cuda.synchronize()
    assert sd.cg_flavour() == 0
    its, _ = sd.last_inner_stats()
    assert its == 10
    sd.set_local_precision(schwz.capi.PRECISION_F64)
    sd.local_solve()
    sd.restrict()
    torch.cuda.synchronize()
    assert sd.local_precision() == schwz.capi.PRECISION_F64
    assert sd.cg_flavour() == flavour
    assert sd.y_form() in (y_form, 1, 2) and (y_form == 0) == (sd.y_form() == 0)
    its, _ = sd.last_inner_stats()
    assert its == 10
    x = sd.get_interior()
    assert np.linalg.norm(x - np.asarray(out["solution"])) <= 1e-7 * np.linalg.norm(out["solution"])


def test_setter_refuses_what_has_no_fp32_solver(schwz, torch_cuda):
    for sk, mk in ((dict(local_solver="direct-ginkgo"), dict()), (dict(), dict(local_precond="ilu")),
                   (dict(), dict(local_precond="block-jacobi", precond_max_block_size=4))):
        s = schwz.Settings(laplacian_dim=3, laplacian_shape=(6, 5, 4), **sk)
        m = schwz.Metadata(num_subdomains=1, tolerance=1e-8, max_iters=50, **mk)
        solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(1), quiet=True)
        solver.initialize()
        sd = solver.subdomains[0]
        with pytest.raises(schwz.NotImplementedSchwz):
            sd.set_local_precision(schwz.capi.PRECISION_F32)
        assert sd.local_precision() == schwz.capi.PRECISION_F64
        with pytest.raises(schwz.SchwzError) as e:
            sd.set_local_precision(7)
        assert e.value.code == schwz.capi.ERR_INVALID


# ---- 9. C++ mirror ----------------------------------------------------------------------------------------------

def _driver(nranks, *args):
    if not os.path.exists(DRIVER):
        pytest.skip("mixed_driver not built (`make -C schwarz-lib_amd mixed_driver`, needs MPI)")
    if not os.path.exists(MPIEXEC):
        pytest.skip("no mpiexec on this machine")
    cmd = [MPIEXEC, "-n", str(nranks), DRIVER] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_mirror_single_precision_converges(oracle):
    import scipy.sparse.linalg as sl
    p = _driver(2, "single", "block-jacobi", 32, 1e-8, 300)
    assert p.returncode == 0, p.stdout + p.stderr
    res = re.search(r"RESULT iters=(\d+) solnorm=([0-9.eE+-]+)", p.stdout)
    assert res, p.stdout
    assert 0 < int(res.group(1)) < 300
    A = _csr(*oracle.laplacian2d(32))
    x = sl.spsolve(A.tocsc(), np.ones(A.shape[0]))
    assert abs(float(res.group(2)) - np.linalg.norm(x)) <= 1e-6 * np.linalg.norm(x)


def test_mirror_refuses_single_with_ilu():
    p = _driver(1, "single", "ilu", 32, 1e-8, 300)
    assert p.returncode == 3, p.stdout + p.stderr
    assert "REFUSED" in p.stdout
