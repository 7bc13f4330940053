"""Compressed-basis GMRES on the device (csrc/gmres.hip, SCHWZ_GMRES_BASIS_F32) through schwz_gmres_solve, against
the restatement of tests/hp_gmres_cb.py in np.longdouble and float64 (tests/gmres_cb_cases.py: the cases, their
sizes and why, the references computed once per process).

No parity of x with the restatement is asserted: a one-ulp fp64 difference in w / ||w|| can flip an fp32 rounding of a
basis vector, which legitimately moves later iterates at the 2^-24 level.  Per case:
  (a) the true relative residual of the returned x, recomputed in np.longdouble, is at most factor * target: target
      is the tolerance (or, where max_iters ended the solve, the recurred norm the longdouble restatement was left
      with), factor the restatement's own ratio of true to recurred residual on that case, doubled, at least two --
      the stop inside a cycle is on the recurred norm;
  (a') and at most 1.01 * (reported + 2^-24 beta): the start residual r of a cycle is represented as
      beta fl32(r / beta) + e with |e| <= 2^-24 beta, and e is outside what the cycle minimises
      (hp_gmres_cb.cycle_bound; beta is the start residual of the restatement's last cycle, doubled for the
      difference between the device's cycle and the restatement's);
  (b) the iteration count is the longdouble restatement's within 1 + SPREAD, SPREAD the largest difference between
      the float64 and longdouble restatements over the cases (0: gmres_cb_cases.SPREAD);
  (c) the reported resnorm against the true residual: true <= factor * reported + the e term of (a'), and
      reported <= factor * true + the e term;
  (d) two runs give the same bits.
One case runs on a non-default stream (tests/stream_rig.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gmres_cb_cases as cc
import hp_gmres_cb
import hp_reference as hp
import stream_rig as rig

pytestmark = pytest.mark.gpu

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPIEXEC = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
DRIVER = os.path.join(ROOT, "schwarz-lib_amd", "build", "gmres_basis_driver")
E32 = 2.0 ** -24


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _solve(torch, g, b, x0, rtol, maxit):
    d_b, d_x = _dev(torch, b), _dev(torch, x0 if x0 is not None else np.zeros(len(b)))
    it, rn = g.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, maxit)
    return d_x.cpu().numpy(), it, rn


def _f32(schwz, A, pc, m):
    return schwz.Gmres(A, pc, 1, m, basis=schwz.capi.GMRES_BASIS_F32)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_compressed_basis_solve(schwz, torch_cuda, case):
    kind, size, m, pc, rtol, maxit = case
    r = cc.ref(case)
    A = schwz.Csr(r.rp, r.col, r.val)
    g = _f32(schwz, A, pc, m)
    assert schwz.capi.lib.schwz_gmres_basis(g.h) == schwz.capi.GMRES_BASIS_F32
    x, it, rn = _solve(torch_cuda, g, r.b, r.x0, rtol, maxit)
    true = hp_gmres_cb.true_relres(r.rp, r.col, r.val, x, r.b, r.x0)
    e_term = 2.0 * E32 * r.beta_last / r.r0 if r.r0 > 0 else 0.0
    print("%s: device %d iterations (longdouble %d, float64 %d), reported %.3e, true %.3e; restatement recurred %.3e "
          "true %.3e, factor %.3g, target %.3e, e term %.3e" %
          (cc.case_id(case), it, r.iters, r.iters64, rn / r.r0 if r.r0 else rn, true, r.recurred, r.true, r.factor,
           r.target, e_term))
    assert np.isfinite(x).all() and np.isfinite(rn)
    assert abs(r.iters64 - r.iters) <= cc.SPREAD
    # (a)
    assert true <= r.factor * r.target
    reported = rn / r.r0 if r.r0 > 0 else rn
    assert true <= 1.01 * (reported + e_term)
    # (b)
    assert abs(it - r.iters) <= 1 + cc.SPREAD
    # (c)
    assert true <= r.factor * reported + e_term
    assert reported <= r.factor * true + e_term
    # (d)
    x2, it2, rn2 = _solve(torch_cuda, g, r.b, r.x0, rtol, maxit)
    assert (it2, rn2) == (it, rn) and rig.same(x, x2)
    fresh = _f32(schwz, A, pc, m)
    x3, it3, rn3 = _solve(torch_cuda, fresh, r.b, r.x0, rtol, maxit)
    assert (it3, rn3) == (it, rn) and rig.same(x, x3)


@pytest.mark.parametrize("kind,size,m,pc,iters", [("cd", 33, 9, 1, 14), ("cd", 33, 30, 1, 30), ("cd", 33, 30, 1, 37),
                                                  ("tri", 1025, 9, 0, 14)])
def test_recurred_norm_tells_what_the_residual_checks_cannot(schwz, torch_cuda, kind, size, m, pc, iters):
    """Two mistakes stay inside the method's own 2^-24 noise, where no residual-based check can see them: an h' that
    is not added into H, and the unrounded v handed to the product.  Both move the recurred norm of a fixed number
    of vectors by a few 1e-9 relative, while float64 rounding moves it by 1e-15.  The tolerance is taken from the
    restatement alone: a quarter of the smaller of the two shifts, each obtained by running the longdouble restatement
    with that mistake switched on; the case must separate that from 32 times the float64-longdouble difference, or it
    fails as not discriminating.  (This is a comparison of one scalar, not of x.  A single flipped fp32 rounding in a
    basis vector -- possible where a one-ulp fp64 difference straddles a rounding boundary, about 1e-4 likely over
    a case of this size -- moves one of >= 1025 entries by one fp32 ulp, a tenth of what the mistakes move.)"""
    rp, col, val = cc.matrix(kind, size)
    n = len(rp) - 1
    b, x0 = cc.rhs(n)
    rec = {}
    for tag, dt, kw in (("ld", LD, {}), ("f64", np.float64, {}), ("no_h2", LD, dict(add_second=False)),
                        ("unrounded", LD, dict(rounded_to_spmv=False))):
        M = hp.precond_jacobi(rp, col, val, dt) if pc == 1 else hp.precond_none(dt)
        _, h = hp_gmres_cb.gmres_cb(rp, col, val, b, x0, M, iters, m, 0.0, dt, **kw)
        assert len(h) - 1 == iters
        rec[tag] = LD(h[-1])

    def rel(a):
        return float(abs(a - rec["ld"]) / rec["ld"])
    tol = min(rel(rec["no_h2"]), rel(rec["unrounded"])) / 4
    noise = 32 * max(rel(rec["f64"]), iters * 2.0 ** -52)
    g = _f32(schwz, schwz.Csr(rp, col, val), pc, m)
    x, it, rn = _solve(torch_cuda, g, b, x0, 0.0, iters)
    print("%s%d m = %d, %d vectors: recurred norm off by %.2e; without h' %.2e, unrounded v %.2e, float64 %.2e" %
          (kind, size, m, iters, rel(LD(rn)), rel(rec["no_h2"]), rel(rec["unrounded"]), rel(rec["f64"])))
    assert tol >= 8 * noise, "the case does not discriminate"
    assert it == iters
    assert rel(LD(rn)) <= tol


def test_the_fp64_basis_is_untouched_by_the_new_entry_point(schwz, torch_cuda, convdiff):
    """schwz_gmres_create_basis with SCHWZ_GMRES_BASIS_F64 is schwz_gmres_create: the same bits."""
    rp, col, val = convdiff(17)
    n = len(rp) - 1
    b, x0 = cc.rhs(n)
    A = schwz.Csr(rp, col, val)
    h = C.c_void_p()
    c = schwz.capi
    c.check(c.lib.schwz_gmres_create_basis(A.h, 1, 1, 9, 0, 0, c.GMRES_BASIS_F64, C.byref(h)))
    via = schwz.Gmres.__new__(schwz.Gmres)
    via.csr, via.h = A, h
    assert c.lib.schwz_gmres_basis(h) == c.GMRES_BASIS_F64
    old = schwz.Gmres(A, 1, 1, 9)
    xa, ia, ra = _solve(torch_cuda, old, b, x0, 1e-8, 100)
    xb, ib, rb = _solve(torch_cuda, via, b, x0, 1e-8, 100)
    assert (ia, ra) == (ib, rb) and rig.same(xa, xb)
    # and the compressed basis is another computation
    xc, ic, rc = _solve(torch_cuda, _f32(schwz, A, 1, 9), b, x0, 1e-8, 100)
    assert not rig.same(xa, xc)
    assert abs(ic - ia) <= 1


# ---- edges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 257, 1025])
def test_max_iters_zero_leaves_x_alone(schwz, torch_cuda, n):
    rp, col, val = cc.tridiag(n)
    b, x0 = cc.rhs(n)
    g = _f32(schwz, schwz.Csr(rp, col, val), 0, 9)
    x, it, rn = _solve(torch_cuda, g, b, x0, 1e-8, 0)
    assert it == 0 and np.array_equal(x, x0)
    r = b.astype(LD) - hp.spmv(rp, col, val, x0)
    assert abs(rn - float(np.sqrt(hp.dot(r, r)))) <= 64 * 2.0 ** -52 * rn


@pytest.mark.parametrize("n", [1, 257])
def test_zero_right_hand_side(schwz, torch_cuda, n):
    rp, col, val = cc.tridiag(n)
    g = _f32(schwz, schwz.Csr(rp, col, val), 0, 8)
    x, it, rn = _solve(torch_cuda, g, np.zeros(n), None, 1e-8, 20)
    assert (it, rn) == (0, 0.0) and not x.any()


def _identity(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n)


@pytest.mark.parametrize("n,scale", [(16, 1.0), (256, 3.0), (4 ** 5, 0.25)])
def test_identity_with_a_basis_fp32_holds_exactly(schwz, torch_cuda, n, scale):
    """A = I, b = +-scale with n a power of 4: beta = scale sqrt(n) and r / beta = +-2^-k exactly, in any summation
    order, so v_0 is not moved by the rounding, w = v_0, h = 1, w - h v_0 = 0 exactly, ||w|| = 0 at j = 0: one
    Krylov vector, resn = 0 and x = b exactly, the result of the fp64 basis."""
    b = scale * np.random.default_rng(n).choice([-1.0, 1.0], n)
    A = schwz.Csr(*_identity(n))
    x, it, rn = _solve(torch_cuda, _f32(schwz, A, 0, 9), b, None, 1e-12, 20)
    assert (it, rn) == (1, 0.0)
    assert np.array_equal(x, b)
    x64, it64, rn64 = _solve(torch_cuda, schwz.Gmres(A, 0, 1, 9), b, None, 1e-12, 20)
    assert (it64, rn64) == (1, 0.0) and np.array_equal(x64, x)


@pytest.mark.parametrize("n", [3, 257])
def test_identity_with_a_general_right_hand_side(schwz, torch_cuda, n):
    """A = I and a b whose normalisation fp32 does not hold: the first cycle leaves the 2^-24 part of b that v_0
    lost, stops on the recurred norm, and the answer is b to that level; a second solve from there (what a restart
    or the next outer iteration is) leaves 2^-24 of that again."""
    b = np.random.default_rng(n).standard_normal(n)
    A = schwz.Csr(*_identity(n))
    g = _f32(schwz, A, 0, 9)
    x, it, rn = _solve(torch_cuda, g, b, None, 1e-12, 20)
    nb = float(np.linalg.norm(b))
    err = float(np.linalg.norm(x - b)) / nb
    print("n = %d: %d iterations, reported %.3e, |x - b| / |b| = %.3e" % (n, it, rn / nb, err))
    assert it <= 2 and err <= 1.01 * (rn / nb + E32)
    x2, it2, rn2 = _solve(torch_cuda, g, b, x, 1e-12, 20)
    err2 = float(np.linalg.norm(x2 - b)) / nb
    assert err2 <= 1.01 * (rn2 / nb + E32 * err) + 4 * 2.0 ** -52


def test_stop_in_mid_cycle_and_max_iters_inside_a_cycle(schwz, torch_cuda):
    """The cases above stop where they stop; here it is asserted that both kinds of stop occur: cd17-m30 reaches
    1e-8 in its third cycle (not at a cycle end), and the same solve capped at 37 = 30 + 7 vectors stops there, with
    the same bits as the first 37 vectors of a longer run would have left (the capped run is its own reference:
    fixed work, twice)."""
    case = ("cd", 17, 30, 1, 1e-8, 100)
    r = cc.ref(case)
    assert r.iters % 30 != 0 and r.iters > 60 and r.recurred <= 1e-8
    g = _f32(schwz, schwz.Csr(r.rp, r.col, r.val), 1, 30)
    x, it, rn = _solve(torch_cuda, g, r.b, r.x0, 1e-8, 100)
    assert it % 30 != 0 and abs(it - r.iters) <= 1 + cc.SPREAD and rn <= 1e-8 * r.r0
    xa, ita, rna = _solve(torch_cuda, g, r.b, r.x0, 1e-8, 37)
    xb, itb, rnb = _solve(torch_cuda, g, r.b, r.x0, 0.0, 37)
    assert ita == itb == 37 and rna == rnb and rig.same(xa, xb)
    assert rna > 1e-8 * r.r0


def test_on_a_non_default_stream(schwz, torch_cuda, convdiff):
    """Two cycles of GMRES(9) with the fp32 basis (9 + 5 vectors: every kernel of the path, a group boundary, the
    cycle end) gated on a stream of its own: bit for bit the default-stream run, and returned while the gate was
    shut."""
    rp, col, val = convdiff(33)
    n = len(rp) - 1
    b, x0 = cc.rhs(n)

    def body(r):
        g = r.hold(_f32(schwz, r.hold(schwz.Csr(rp, col, val)), 1, 9))
        d_b, d_x = r.input(b), r.input(x0)
        r.arm()
        r.call(g.solve, d_b.data_ptr(), d_x.data_ptr(), 0.0, 14, stream=r.handle, want_stats=False,
               label="Gmres(9, fp32 basis).solve")
        r.snap(d_x)
        return None
    (x,), _ = rig.both(torch_cuda, body, "gmres fp32 basis")
    assert np.isfinite(x).all() and not np.array_equal(x, x0)


# ---- inside RAS -------------------------------------------------------------------------------------------------

def _write_mtx(path, rp, col, val):
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, rp[-1]))
        for r, c, v in zip(rows, col, val):
            f.write("%d %d %.17g\n" % (r + 1, c + 1, v))
    return path


def _ras(schwz, path, P, basis, **kw):
    s = schwz.Settings(matrix_filename=path, explicit_laplacian=False, non_symmetric_matrix=True, restart_iter=10,
                       **kw)
    m = schwz.Metadata(num_subdomains=P, gmres_basis=basis, local_precond="block-jacobi", precond_max_block_size=1,
                       local_solver_tolerance=1e-12, tolerance=1e-8, max_iters=400)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    return solver, m


def test_ras_run_with_the_compressed_basis(schwz, torch_cuda, convdiff, tmp_path):
    rp, col, val = convdiff(30)
    n = len(rp) - 1
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    P = 3
    c = schwz.capi
    single, m = _ras(schwz, path, P, "single")
    assert all(sd.gmres_basis() == c.GMRES_BASIS_F32 and sd.nonsym_solver() == c.NONSYM_GMRES
               for sd in single.subdomains.values())
    out = single.run()
    double, _ = _ras(schwz, path, P, "double")
    assert all(sd.gmres_basis() == c.GMRES_BASIS_F64 for sd in double.subdomains.values())
    ref = double.run()
    x = np.asarray(out["solution"], dtype=LD)
    res = np.ones(n, dtype=LD) - hp.spmv(rp, col, val, x)
    rel = float(np.sqrt(hp.dot(res, res)) / np.sqrt(LD(n)))
    print("P = %d: %d outer iterations (fp64 basis %d), true relative residual %.3e" %
          (P, out["iter_count"], ref["iter_count"], rel))
    assert out["converged"] and ref["converged"]
    assert rel <= m.tolerance
    assert abs(out["iter_count"] - ref["iter_count"]) <= 1


def test_subdomain_setter(schwz, torch_cuda, convdiff):
    """The setter round-trips, is remembered across BiCGSTAB, refuses what it must, and the local solve of a
    subdomain with neighbours is schwz_gmres_solve with that basis on the local matrix: the same bits."""
    torch, c = torch_cuda, schwz.capi
    rp, col, val = convdiff(30)
    P, me = 3, 1
    prob = schwz.Problem.from_csr(rp, col, val)
    sd = schwz.Subdomain(prob, P, me, 2, schwz.partition_regular(prob.N, P))
    nloc = sd.local_size_x
    rng = np.random.default_rng(5)
    sd.to_device(rng.standard_normal(nloc), precond=c.PRECOND_JACOBI, local_tol=0.0, local_max_iters=12,
                 non_symmetric=True, restart_iter=9)
    assert sd.gmres_basis() == c.GMRES_BASIS_F64
    sd.set_gmres_basis(c.GMRES_BASIS_F32)
    sd.set_gmres_basis(c.GMRES_BASIS_F32)
    assert sd.gmres_basis() == c.GMRES_BASIS_F32 and sd.nonsym_solver() == c.NONSYM_GMRES
    sd.set_gmres_basis(c.GMRES_BASIS_F64)
    assert sd.gmres_basis() == c.GMRES_BASIS_F64
    sd.set_nonsym_solver(c.NONSYM_BICGSTAB)
    sd.set_gmres_basis(c.GMRES_BASIS_F32)              # remembered while BiCGSTAB is set
    assert sd.gmres_basis() == c.GMRES_BASIS_F32 and sd.nonsym_solver() == c.NONSYM_BICGSTAB
    sd.set_nonsym_solver(c.NONSYM_GMRES)
    assert sd.gmres_basis() == c.GMRES_BASIS_F32 and sd.nonsym_solver() == c.NONSYM_GMRES
    with pytest.raises(schwz.SchwzError) as e:
        sd.set_gmres_basis(2)
    assert e.value.code == c.ERR_INVALID

    nx = nloc + sd.halo_size
    idx = torch.arange(nx, dtype=torch.int32, device="cuda")

    def get(which):
        p, cnt = sd.vector(which)
        t = torch.empty(cnt, dtype=torch.float64, device="cuda")
        schwz.gather(cnt, idx.data_ptr(), p, t.data_ptr())
        torch.cuda.synchronize()
        return t.cpu().numpy()

    def put(which, a):
        p, cnt = sd.vector(which)
        assert len(a) == cnt
        t = _dev(torch, a)
        schwz.gather(cnt, idx.data_ptr(), t.data_ptr(), p)
        torch.cuda.synchronize()

    put(0, rng.standard_normal(nx))
    put(2, rng.standard_normal(nloc) * 0.1)
    sd.update_boundary()
    torch.cuda.synchronize()
    bt, y0 = get(1), get(2)
    h = C.c_void_p()
    c.check(c.lib.schwz_ras_local_csr(sd.h, C.byref(h)))

    class _Handle:
        def __init__(self, h):
            self.h = h
    alone = schwz.Gmres(_Handle(h), c.PRECOND_JACOBI, 1, 9, basis=c.GMRES_BASIS_F32)
    assert sd.local_solve(want_iters=True) == 12
    torch.cuda.synchronize()
    exp, it, rn = _solve(torch, alone, bt, y0, 0.0, 12)
    assert it == 12 and np.array_equal(get(2), exp)
    assert sd.last_inner_stats() == (12, rn)
    # a symmetric subdomain has no such choice
    sd2 = schwz.Subdomain(prob, P, me, 2, schwz.partition_regular(prob.N, P))
    sd2.to_device(np.ones(nloc), precond=c.PRECOND_JACOBI)
    with pytest.raises(schwz.NotImplementedSchwz):
        sd2.set_gmres_basis(c.GMRES_BASIS_F32)
    assert sd2.gmres_basis() == c.GMRES_BASIS_F64


# ---- the C++ mirror ---------------------------------------------------------------------------------------------

def _driver(nranks, *args):
    if not os.path.exists(DRIVER):
        pytest.skip("gmres_basis_driver not built (`make -C schwarz-lib_amd gmres_basis_driver`, needs MPI)")
    if not os.path.exists(MPIEXEC):
        pytest.skip("no mpiexec on this machine")
    cmd = [MPIEXEC, "-n", str(nranks), DRIVER] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_mirror_runs_the_compressed_basis_like_the_python_host(schwz, torch_cuda, convdiff, tmp_path):
    rp, col, val = convdiff(30)
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    P = 2
    p = _driver(P, "single", path, 1e-8, 400, 10)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "with restart iter 10 (fp32 basis)" in p.stdout
    res = re.search(r"RESULT iters=(\d+) solnorm=([0-9.eE+-]+)", p.stdout)
    final = re.search(r"^ residual norm ([0-9.eE+-]+)$", p.stdout, re.M)
    assert res and final, p.stdout
    solver, m = _ras(schwz, path, P, "single", overlap=2)
    out = solver.run()
    assert out["converged"]
    assert int(res.group(1)) == out["iter_count"]
    print("mirror: %s iterations, final residual %s; python host: %d, %.17g" %
          (res.group(1), final.group(1), out["iter_count"], out["residual_norm"]))
    assert abs(float(final.group(1)) - out["residual_norm"]) <= 1e-10 * out["residual_norm"]
    norm = float(np.linalg.norm(out["solution"]))
    assert abs(float(res.group(2)) - norm) <= 1e-10 * norm
    # the double run through the mirror: no mention of the basis, an outer count within one
    q = _driver(P, "double", path, 1e-8, 400, 10)
    assert q.returncode == 0 and "fp32 basis" not in q.stdout
    res_d = re.search(r"RESULT iters=(\d+)", q.stdout)
    assert abs(int(res_d.group(1)) - int(res.group(1))) <= 1
    # no effect with BiCGSTAB
    q = _driver(P, "single", path, 1e-8, 400, 10, "bicgstab")
    assert q.returncode == 0 and "(BiCGSTAB)" in q.stdout and "fp32 basis" not in q.stdout


def test_mirror_refuses_an_unknown_basis_name(convdiff, tmp_path):
    rp, col, val = convdiff(6)
    path = _write_mtx(str(tmp_path / "cd.mtx"), rp, col, val)
    p = _driver(1, "half", path, 1e-8, 10, 1)
    assert p.returncode == 3, p.stdout + p.stderr
    assert "REFUSED" in p.stdout
