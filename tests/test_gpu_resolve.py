"""One matrix, many right-hand sides on the GPU: schwz_ras_rhs_set / _index / _gather / _aggregate / _norm_sq,
schwz_ras_restart and SolverRAS.set_rhs / solve.

  1. the kernels, bit for bit against numpy (the norm: against an extended-precision sum);
  2. restart(keep_x = 0) after three steps leaves what a fresh upload leaves, in the unified and in the separate form;
  3. THE IDENTITY: initialize(b1), run(), set_rhs(b2), run() computes what initialize(b2), run() computes -- the same
     iteration count, the same residual histories, the same solution, bit for bit -- for every local solver, coding,
     precision, exchange and level this build has.  A failure here means that some state which depends on b, or on
     the solve before, survived set_rhs;
  4. a device tensor as right-hand side gives the bits of the same values as a host array;
  5. initial_guess = "keep";
  6. the new entry points on a non-default stream (stream_rig.py).

Everything at toy size.  All comparisons between runs are exact: the library folds every reduction in a fixed order."""
import math
import os

import numpy as np
import pytest

import stream_rig as rig
import test_gpu_ras_steps as steps

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
LAP = (16, 10, 7)           # lap3d_16x10x7: 1120 rows
N_LAP = 16 * 10 * 7
WALK_ENV = {"SCHWZ_SPMV_PATTERN": "2", "SCHWZ_SPMV_PAIR": "2", "SCHWZ_SPMV_SWEEP": "2", "SCHWZ_SWEEP_T": "512",
            "SCHWZ_CG_DEFERX": "2"}


def _read(schwz, torch, ptr, n):
    """n doubles at the device address ptr."""
    idx = torch.arange(max(n, 1), dtype=torch.int32, device="cuda")
    t = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    schwz.gather(n, idx.data_ptr(), ptr, t.data_ptr())
    torch.cuda.synchronize()
    return t.cpu().numpy()[:n]


def _vec(schwz, torch, sd, which):
    return _read(schwz, torch, *sd.vector(which))


def _on_device(schwz, prob, P, fr, rhs_global, **kw):
    """The subdomains of a partition, connected and uploaded with rhs_global in their local order."""
    sds = [schwz.Subdomain(prob, P, me, 2, fr) for me in range(P)]
    for me, lst in schwz.InProcessComm(P).handshake({me: sd.get_lists() for me, sd in enumerate(sds)}).items():
        for q, ids in lst:
            sds[me].add_put_list(q, ids)
    for sd in sds:
        sd.to_device(rhs_global[sd.local_to_global[:sd.local_size_x]], precond=schwz.capi.PRECOND_JACOBI, **kw)
    return sds


def _special(n, seed):
    """Values whose bits a copy must keep: signed zeros, denormals, huge and tiny magnitudes among normal ones."""
    v = np.random.default_rng(seed).standard_normal(n)
    v[::7] = 1.7e308
    v[1::11] = -0.0
    v[2::13] = 5e-324
    v[3::17] = -1e-310
    v[-1] = -2.0 ** -1022
    return v


# ---- 1. kernels ----------------------------------------------------------------------------------------------------

def test_rhs_set_from_the_host_and_from_the_device_keeps_bits_and_pointer(schwz, torch_cuda):
    torch = torch_cuda
    R = steps.StepRig(schwz, torch, "band_p3", {})
    for me, sd in R.sds.items():
        p3, n = sd.vector(3)
        assert n == sd.local_size_x
        before_bt = _vec(schwz, torch, sd, 1)
        v = _special(n, 10 + me)
        sd.rhs_set(v)
        assert rig.same(_vec(schwz, torch, sd, 3), v) and sd.vector(3)[0] == p3
        w = _special(n, 20 + me)[::-1].copy()
        t = torch.from_numpy(w).cuda()
        sd.rhs_set(t.data_ptr())
        assert rig.same(_vec(schwz, torch, sd, 3), w) and sd.vector(3)[0] == p3
        assert rig.same(_vec(schwz, torch, sd, 1), before_bt)      # b~ is restart's business


@pytest.mark.parametrize("permuted", [False, True], ids=["own_l2g", "graph_partition_permutation"])
def test_rhs_gather_equals_numpy_indexing(schwz, torch_cuda, permuted):
    """lap3d_16x10x7, 3 subdomains, overlap 2.  Without a permutation: contiguous parts of 30 / 545 / 545 rows --
    local_size_x 76 (one workgroup, below 256), 735 and 705 (odd: no multiple of 4, more than one workgroup) -- and
    the subdomain's own local-to-global list as the map.  With the graph partition: the composed map
    permutation[local_to_global], as SolverRAS._rhs indexes a caller's right-hand side."""
    torch = torch_cuda
    prob = schwz.Problem.laplacian(3, *LAP)
    if permuted:
        prob, perm, fr = prob.permute(prob.partition_graph(3), 3)
        perm = np.asarray(perm, dtype=np.int64)
    else:
        perm, fr = None, np.array([0, 30, 575, N_LAP], dtype=np.int64)
    sds = _on_device(schwz, prob, 3, fr, np.ones(N_LAP))
    if not permuted:
        assert [sd.local_size_x for sd in sds] == [76, 735, 705]
    g = _special(N_LAP, 5)
    d_g = torch.from_numpy(g).cuda()
    for sd in sds:
        n = sd.local_size_x
        l2g = sd.local_to_global[:n]
        index = l2g if perm is None else perm[l2g]
        p3 = sd.vector(3)[0]
        if perm is not None:
            sd.rhs_index(index)
        sd.rhs_gather(d_g.data_ptr(), N_LAP)
        assert rig.same(_vec(schwz, torch, sd, 3), g[index]) and sd.vector(3)[0] == p3
        # another map, then back to the own list: the uploaded map is replaced, not reused
        rev = index[::-1].copy()
        sd.rhs_index(rev)
        sd.rhs_gather(d_g.data_ptr(), N_LAP)
        assert rig.same(_vec(schwz, torch, sd, 3), g[rev])
        sd.rhs_index(None)
        sd.rhs_gather(d_g.data_ptr(), N_LAP)
        assert rig.same(_vec(schwz, torch, sd, 3), g[l2g])
        # refusals: an index outside [0, N), a global vector of another length; the map in force stays
        for bad in (-1, N_LAP):
            wrong = index.copy()
            wrong[n // 2] = bad
            with pytest.raises(schwz.SchwzError) as e:
                sd.rhs_index(wrong)
            assert e.value.code == schwz.capi.ERR_INVALID
        with pytest.raises(schwz.SchwzError) as e:
            sd.rhs_gather(d_g.data_ptr(), N_LAP - 1)
        assert e.value.code == schwz.capi.ERR_INVALID
        sd.rhs_gather(d_g.data_ptr(), N_LAP)
        assert rig.same(_vec(schwz, torch, sd, 3), g[l2g])


def test_rhs_norm_sq_against_an_extended_precision_sum(schwz, torch_cuda):
    """Interior rows only (and all local rows for the _local form), to 1e-14 relative: the device sums at most
    ceil(n / 512) squares per lane and folds 256 lanes and the workgroups in trees -- a few dozen roundings of 2^-53."""
    torch = torch_cuda
    R = steps.StepRig(schwz, torch, "band_p3", {})
    for me, sd in R.sds.items():
        v = np.random.default_rng(70 + me).standard_normal(sd.local_size_x) * 10.0 ** np.random.default_rng(80 + me).integers(
            -3, 4, sd.local_size_x)
        sd.rhs_set(v)
        for got, rows in ((sd.rhs_norm_sq(), sd.local_size), (sd.rhs_norm_sq_local(), sd.local_size_x)):
            ref = math.fsum(float(np.longdouble(x) * np.longdouble(x)) for x in v[:rows])
            print("rhs_norm_sq subdomain %d rows %d: %.17g ref %.17g rel %.2e" % (me, rows, got, ref, abs(got - ref) / ref))
            assert abs(got - ref) <= 1e-14 * ref
    assert sd.local_size < sd.local_size_x


def _aggregate_vector():
    """One aggregate id per global row of lap3d_16x10x7: an aggregate of ONE row, one of more than 256 rows (a lane's
    loop far longer than its neighbours'), the rest in runs of 37 rows; rows of one id in different subdomains become
    different aggregates (the host layer splits them)."""
    agg = 2 + np.arange(N_LAP) // 37
    agg[5] = 0
    agg[40:340] = 1
    return agg


@pytest.mark.parametrize("P", [1, 3])
def test_rhs_aggregate_gives_the_beta_of_a_fresh_plan(schwz, torch_cuda, P):
    """beta is read through the coarse residual of x~ = 0, s = beta - 0.  Against a fresh initialize() on the same b
    (the host plan) and against a plain Python loop over each aggregate's rows in ascending order."""
    torch = torch_cuda
    agg = _aggregate_vector()
    rng = np.random.default_rng(17)
    b1, b2 = rng.standard_normal(N_LAP), rng.standard_normal(N_LAP) * 10.0 ** rng.integers(-6, 7, N_LAP)

    def make(b):
        s = schwz.Settings(laplacian_dim=3, laplacian_shape=LAP)
        m = schwz.Metadata(num_subdomains=P, coarse_space="aggregates", coarse_aggregate_vector=agg, max_iters=3)
        solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
        solver.initialize(rhs=b)
        return solver

    def s_of(solver):
        obj = solver._coarse["obj"]
        for sd in solver.subdomains.values():
            sd.coarse_residual(obj)
        ptr, nc = obj.vector(0)
        return _read(schwz, torch, ptr, nc)
    a = make(b1)
    a.run()
    a.set_rhs(b2)
    fresh = make(b2)
    got, want = s_of(a), s_of(fresh)
    assert rig.same(got, want), np.nonzero(got != want)
    # the plain loop, per (subdomain, caller's id) in the order the host layer numbers them
    fr = np.asarray(a.metadata.first_row)
    sums = []
    for p in range(P):
        ids = agg[fr[p]:fr[p + 1]]
        for a_id in np.unique(ids):
            t = 0.0
            for i in np.nonzero(ids == a_id)[0]:
                t += b2[fr[p] + i]
            sums.append(t)
    assert rig.same(got, np.array(sums))
    sizes = [int(np.sum(agg[fr[p]:fr[p + 1]] == k)) for p in range(P) for k in np.unique(agg[fr[p]:fr[p + 1]])]
    assert min(sizes) == 1 and max(sizes) > 256


# ---- 2. restart = fresh -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["unified", "separate"])
def test_restart_after_three_steps_leaves_what_a_fresh_upload_leaves(schwz, torch_cuda, monkeypatch, form):
    """Unified: one subdomain, CG with the x update deferred at every size (SCHWZ_CG_DEFERX=2), y lives in the x~
    buffers.  Separate: three subdomains.  Vectors 0 - 3, schwz_ras_y_form and the inner statistics."""
    torch = torch_cuda
    monkeypatch.setenv("SCHWZ_CG_DEFERX", "2")
    P = 1 if form == "unified" else 3
    b = np.random.default_rng(3).standard_normal(N_LAP)

    def make():
        s = schwz.Settings(laplacian_dim=3, laplacian_shape=LAP)
        m = schwz.Metadata(num_subdomains=P, tolerance=1e-12, max_iters=50, local_precond="block-jacobi",
                           precond_max_block_size=1, local_solver_tolerance=0.0, local_max_iters=5)
        solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
        solver.initialize(rhs=b)
        return solver
    used, fresh = make(), make()
    used.begin_run()
    for _ in range(3):
        assert not used.step()
    torch.cuda.synchronize()
    for me in range(P):
        sd, sf = used.subdomains[me], fresh.subdomains[me]
        assert np.abs(_vec(schwz, torch, sd, 0)).max() > 0 and sd.last_inner_stats()[0] == 5
        p1, p3 = sd.vector(1)[0], sd.vector(3)[0]
        sd.restart(False)
        torch.cuda.synchronize()
        assert sd.y_form() == sf.y_form() == (1 if form == "unified" else 0)
        for which in range(4):
            assert rig.same(_vec(schwz, torch, sd, which), _vec(schwz, torch, sf, which)), (me, which)
        assert (sd.vector(1)[0], sd.vector(3)[0]) == (p1, p3)
        assert sd.last_inner_stats() == sf.last_inner_stats() == (0, 0.0)
        assert sd.cg_flavour() == sf.cg_flavour() == 0
        with pytest.raises(schwz.SchwzError) as e:
            schwz.capi.check(schwz.capi.lib.schwz_ras_restart(sd.h, 2, None))
        assert e.value.code == schwz.capi.ERR_INVALID


# ---- 3. the identity -------------------------------------------------------------------------------------------------------

def _ani4():
    g = np.load(os.path.join(G, "ani4_crop.npz"))
    return g["rp"].astype(np.int64), g["col"], g["val"]


def _overlapped(s):
    s.comm_settings.enable_onesided = True
    s.comm_settings.enable_overlap = True
    s.convergence_settings.enable_decentralized_leader_election = True


JACOBI = dict(local_precond="block-jacobi", precond_max_block_size=1)
FIXED10 = dict(JACOBI, local_solver_tolerance=0.0, local_max_iters=10)
NONSYM = dict(non_symmetric_matrix=True, restart_iter=10)
# name -> (matrix, settings, metadata, subdomain counts, environment, settings hook)
CASES = {
    "jacobi_cg10_fixed": ("lap16", {}, FIXED10, (1, 3), {}, None),
    "jacobi_cg10_tolerance": ("lap12", {}, dict(JACOBI, local_solver_tolerance=1e-3, local_max_iters=10), (1, 3), {}, None),
    "z_sweep_walk": ("slab", {}, dict(JACOBI, local_solver_tolerance=0.0, local_max_iters=7, tolerance=1e-5), (1, 3),
                     WALK_ENV, None),
    "codings_off": ("lap16", dict(spmv_variant=6), FIXED10, (1, 3), {}, None),
    "deferred_x_lazy_tail": ("lap16", {}, FIXED10, (1, 3), {"SCHWZ_CG_DEFERX": "2"}, None),
    "block_jacobi_4": ("lap12", {}, dict(local_precond="block-jacobi", precond_max_block_size=4,
                                         local_solver_tolerance=1e-10), (1, 3), {}, None),
    "ilu": ("lap12", {}, dict(local_precond="ilu", local_solver_tolerance=1e-10), (1, 3), {}, None),
    "isai": ("lap12", {}, dict(local_precond="isai", local_solver_tolerance=1e-10), (1, 3), {}, None),
    "single_precision": ("lap16", {}, dict(FIXED10, local_solver_precision="single"), (1, 3), {}, None),
    "chebyshev": ("lap16", {}, dict(FIXED10, symmetric_solver="chebyshev"), (1, 3), {}, None),
    # (22 ms per outer iteration, level-scheduled sweeps over three large factors: 30 iterations per run, which none
    # of the runs ends before; the runs that end on their tolerance are the other cases)
    "direct_cholmod_ani4": ("ani4", dict(local_solver="direct-cholmod"), dict(tolerance=1e-8, max_iters=30), (3,), {}, None),
    "gmres": ("convdiff", NONSYM, dict(JACOBI, local_solver_tolerance=1e-11, local_max_iters=600), (1, 3), {}, None),
    "gmres_fp32_basis": ("convdiff", NONSYM, dict(JACOBI, local_solver_tolerance=1e-11, local_max_iters=600,
                                                  gmres_basis="single"), (1, 3), {}, None),
    "bicgstab": ("convdiff", NONSYM, dict(JACOBI, local_solver_tolerance=1e-11, local_max_iters=600,
                                          non_symmetric_solver="bicgstab"), (1, 3), {}, None),
    "umfpack": ("convdiff", dict(non_symmetric_matrix=True, local_solver="direct-ginkgo", factorization="umfpack"), {},
                (1, 3), {}, None),
    "coarse_aggregates": ("lap16", {}, dict(FIXED10, coarse_space="aggregates", coarse_aggregates=4), (1, 3), {}, None),
    "two_stage": ("lap12", dict(reset_local_crit_iter=4), dict(JACOBI, local_solver_tolerance=1e-10, local_max_iters=3,
                                                               updated_max_iters=-1, tolerance=1e-8), (1, 3), {}, None),
    "fp32_halos": ("lap16", dict(use_mixed_precision=True), dict(FIXED10, tolerance=1e-5), (3,), {}, None),
    "overlapped_onesided_model": ("lap16", {}, FIXED10, (3,), {}, _overlapped),
}
SHAPES = {"lap16": LAP, "lap12": (12, 12, 12), "slab": (256, 4, 30)}


def _case_solver(schwz, convdiff, name, P):
    matrix, s_kw, m_kw, _, _, hook = CASES[name]
    s_kw, m_kw = dict(s_kw), dict(dict(tolerance=1e-6, max_iters=400), **m_kw)
    csr = None
    if matrix in SHAPES:
        s_kw.update(laplacian_dim=3, laplacian_shape=SHAPES[matrix])
        n = int(np.prod(SHAPES[matrix]))
    else:
        s_kw.update(explicit_laplacian=False)
        rp, col, val = _ani4() if matrix == "ani4" else convdiff(30)
        csr = (np.asarray(rp, dtype=np.int64), col, val)
        n = len(rp) - 1
    s = schwz.Settings(**s_kw)
    if hook:
        hook(s)
    m = schwz.Metadata(num_subdomains=P, **m_kw)
    return schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True), csr, n


def _history(solver, out):
    ppd = solver.metadata.post_process_data
    return (out["iter_count"], out["converged"], np.array(ppd["local_residual_vector_out"]),
            [np.array(h) for h in ppd["global_residual_vector_out"]], np.array(ppd["local_converged_resnorm"]),
            out["residual_norm"], out["solution"].copy())


def _assert_same_run(a, b, tag):
    assert a[0] == b[0] and a[1] == b[1], (tag, a[0], b[0])
    assert rig.same(a[2], b[2]), tag
    assert len(a[3]) == len(b[3]) and all(rig.same(x, y) for x, y in zip(a[3], b[3])), tag
    assert rig.same(a[4], b[4]), tag
    assert a[5] == b[5], tag
    assert np.array_equal(a[6], b[6]) and rig.same(a[6], b[6]), tag


@pytest.mark.parametrize("name,P", [(k, P) for k, v in CASES.items() for P in v[3]])
def test_a_new_rhs_on_a_used_solver_computes_what_a_fresh_solver_computes(schwz, torch_cuda, convdiff, monkeypatch, name, P):
    for k, v in CASES[name][4].items():
        monkeypatch.setenv(k, v)
    used, csr, n = _case_solver(schwz, convdiff, name, P)
    rng = np.random.default_rng(sum(name.encode()) + P)
    b1, b2 = rng.uniform(0.5, 1.5, n), rng.standard_normal(n)
    used.initialize(matrix=csr, rhs=b1)
    first = used.run()
    assert first["iter_count"] >= 1     # (one subdomain with converged local solves: one outer iteration)
    used.set_rhs(b2)
    again = _history(used, used.run())
    fresh, _, _ = _case_solver(schwz, convdiff, name, P)
    fresh.initialize(matrix=csr, rhs=b2)
    want = _history(fresh, fresh.run())
    print("%s P=%d: first solve %d outer iterations, second %d (fresh %d), converged %s" %
          (name, P, first["iter_count"], again[0], want[0], again[1]))
    _assert_same_run(again, want, (name, P))
    assert again[0] >= 1 and np.isfinite(again[6]).all()
    assert used.result["rhs_norm"] == fresh.result["rhs_norm"]
    if name == "z_sweep_walk":
        assert all(sd.cg_flavour() & 60 == 60 for sd in used.subdomains.values())
    if name == "deferred_x_lazy_tail":
        assert all(sd.cg_flavour() & 4 for sd in used.subdomains.values())
    if name == "direct_cholmod_ani4":
        return
    # ... and a third time, with the first right-hand side again: the solver is as good as new every time
    third = _history(used, used.solve(b1))
    assert third[0] == first["iter_count"] and np.array_equal(third[6], first["solution"]), (name, P)


# ---- 4. a device tensor --------------------------------------------------------------------------------------------------------

def test_a_device_tensor_gives_the_bits_of_the_host_array(schwz, torch_cuda):
    """Three subdomains of the graph partition (a permutation), two levels: gather + aggregate on the device against
    the host path; rhs_norm comes from the device sum there and agrees to rounding."""
    torch = torch_cuda
    rng = np.random.default_rng(44)
    b1, b2 = rng.standard_normal(N_LAP), rng.standard_normal(N_LAP)

    def make():
        s = schwz.Settings(laplacian_dim=3, laplacian_shape=LAP, partition=schwz.PARTITION_METIS)
        m = schwz.Metadata(num_subdomains=3, tolerance=1e-7, max_iters=300, coarse_space="aggregates", coarse_aggregates=3,
                           **FIXED10)
        solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(3), quiet=True)
        solver.initialize(rhs=b1)
        solver.run()
        return solver
    host, dev = make(), make()
    assert host.metadata.permutation is not None
    want = _history(host, host.solve(b2))
    t = torch.from_numpy(b2).cuda()
    got = _history(dev, dev.solve(t))
    _assert_same_run(got, want, "device tensor")
    for me, sd in dev.subdomains.items():
        assert rig.same(_vec(schwz, torch, sd, 3), _vec(schwz, torch, host.subdomains[me], 3))
    assert dev._user_rhs is None and dev._device_rhs is t
    assert abs(dev.result["rhs_norm"] - host.result["rhs_norm"]) <= 1e-14 * host.result["rhs_norm"]
    assert abs(host.result["rhs_norm"] - np.linalg.norm(b2)) <= 1e-14 * np.linalg.norm(b2)
    # back to a host array, and to the default (ones): the tensor is let go
    ones = _history(dev, dev.solve(None))
    assert dev._device_rhs is None and abs(dev.result["rhs_norm"] - np.sqrt(N_LAP)) <= 1e-14 * np.sqrt(N_LAP)
    fresh = schwz.SolverRAS(schwz.Settings(laplacian_dim=3, laplacian_shape=LAP, partition=schwz.PARTITION_METIS),
                            schwz.Metadata(num_subdomains=3, tolerance=1e-7, max_iters=300, coarse_space="aggregates",
                                           coarse_aggregates=3, **FIXED10), comm=schwz.InProcessComm(3), quiet=True)
    fresh.initialize()
    _assert_same_run(ones, _history(fresh, fresh.run()), "ones")


# ---- 5. keep ----------------------------------------------------------------------------------------------------------------

def test_keep_starts_from_the_last_iterate(schwz, oracle, torch_cuda):
    """Tolerance 1e-4 on the sum of the subdomains' residual norms relative to that of a zero start vector -- the
    reference a kept start is measured against too.  The final residual norms against scipy to 1e-10 relative: both
    sides form b - A x with about ten roundings of 2^-53 |a_ij x_j| <= 2^-53 * 12 * 30 per row, which moves the norm of a
    residual of 1e-4 |b| ~ 3e-3 by some 1e-14, i.e. 1e-11 relative."""
    tol, P = 1e-4, 3
    import scipy.sparse as sp
    rp, col, val = oracle.laplacian3d(*LAP)
    A = sp.csr_matrix((val, col, rp), shape=(N_LAP, N_LAP))
    rng = np.random.default_rng(91)
    b1 = rng.uniform(0.5, 1.5, N_LAP)
    b2 = b1 * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, N_LAP))

    def make():
        s = schwz.Settings(laplacian_dim=3, laplacian_shape=LAP)
        m = schwz.Metadata(num_subdomains=P, tolerance=tol, max_iters=400, **FIXED10)
        return schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)

    def check(out, b):
        ref = np.linalg.norm(b - A @ out["solution"])
        print("residual_norm %.17g scipy %.17g rel %.2e, %d iterations" %
              (out["residual_norm"], ref, abs(out["residual_norm"] - ref) / ref, out["iter_count"]))
        assert out["converged"] and abs(out["residual_norm"] - ref) <= 1e-10 * ref
        assert abs(out["rhs_norm"] - np.linalg.norm(b)) <= 1e-14 * np.linalg.norm(b)
        # under the tolerance: the run stops when sum_p l_p <= tol sum_p l0_p, l_p the norm of subdomain p's residual over
        # its interior and overlap rows; the interior rows of l_p are rows of b - A x, so |b - A x| <= sum_p l_p, and
        # l0_p, the same for x = 0, is at most |b|
        assert out["residual_norm"] <= tol * P * np.linalg.norm(b)
    solver = make()
    solver.initialize(rhs=b1)
    first = solver.run()
    check(first, b1)
    same_again = solver.solve(b1, "keep")
    check(same_again, b1)
    assert same_again["iter_count"] < first["iter_count"]
    kept = solver.solve(b2, "keep")
    check(kept, b2)
    zero = solver.solve(b2, "zero")
    check(zero, b2)
    assert kept["iter_count"] < zero["iter_count"], (kept["iter_count"], zero["iter_count"])
    # three solves in a row, alternating
    for k, guess in enumerate(("zero", "keep", "zero")):
        b = b1 * (1.0 + 0.1 * k) if k != 1 else b2
        check(solver.solve(b, guess), b)


# ---- 6. streams ---------------------------------------------------------------------------------------------------------------

def _stream_body(schwz, torch):
    def body(r):
        R = r.hold(steps.StepRig(schwz, torch, "band_p3", {}, maxit=5))
        sds, N = R.sds, R.N
        fr = np.asarray(sds[0].first_row, dtype=np.int64)
        owner = np.searchsorted(fr, np.arange(N), side="right") - 1
        agg = 3 * owner + (3 * (np.arange(N) - fr[owner])) // (fr[owner + 1] - fr[owner])
        obj = r.hold(schwz.Coarse(np.eye(9)))
        g = np.random.default_rng(8).standard_normal(N)
        d_g = r.input(g)
        new, d_new, true_x = {}, {}, {}
        for me, sd in sds.items():
            sd.coarse_set_aggregates(agg[R.l2g[me]], 3 * me, 3, 9)
            sd.local_solve()                               # a solve to forget: statistics, y ahead of x~
            assert sd.last_inner_stats()[0] == 5
            # first uses build and upload their tables (they wait for the stream, once): before the gate
            sd.rhs_aggregate()
            sd.rhs_gather(r.hold(torch.zeros(N, dtype=torch.float64, device="cuda")).data_ptr(), N)
            new[me] = np.random.default_rng(60 + me).standard_normal(sd.local_size_x)
            d_new[me] = r.input(new[me])
            true_x[me] = r.hold(torch.from_numpy(R.x[me]).cuda())
            if r.gated:
                R.put(me, 0, np.full(len(R.x[me]), np.nan))
        r.arm()
        if r.gated:                                        # behind the gate: x~ takes its true values
            for me, sd in sds.items():
                p, cnt = sd.vector(0)
                schwz.gather(cnt, R.idx[me].data_ptr(), true_x[me].data_ptr(), p, stream=r.handle)

        def snap_state(me, ids=(0, 1, 2, 3)):
            for which in ids:
                p, cnt = sds[me].vector(which)
                t = r.output(cnt)
                schwz.gather(cnt, R.idx[me].data_ptr(), p, t.data_ptr(), stream=r.handle)
                r.snap(t)

        def snap_s():
            p, nc = obj.vector(0)
            t = r.output(nc)
            idx = r.hold(torch.arange(nc, dtype=torch.int32, device="cuda"))
            schwz.gather(nc, idx.data_ptr(), p, t.data_ptr(), stream=r.handle)
            r.snap(t)
        for me, sd in sds.items():
            r.call(sd.rhs_set, d_new[me].data_ptr(), stream=r.handle)
            r.call(sd.rhs_aggregate, stream=r.handle)
            r.call(sd.restart, True, stream=r.handle)
            snap_state(me)
            r.call(sd.coarse_residual, obj, stream=r.handle)
        snap_s()
        for me, sd in sds.items():
            r.call(sd.rhs_gather, d_g.data_ptr(), N, stream=r.handle)
            r.call(sd.rhs_aggregate, stream=r.handle)
            r.call(sd.restart, False, stream=r.handle)
            snap_state(me)
            r.call(sd.coarse_residual, obj, stream=r.handle)
        snap_s()
        r.check_shut("rhs_set, rhs_gather, rhs_aggregate and restart of three subdomains, enqueued whole")
        host = []
        for me, sd in sds.items():                         # the calls that hand a value to the host
            host.append(r.call(sd.rhs_norm_sq, stream=r.handle, reads_back=True))
            host.append(r.call(sd.rhs_norm_sq_local, stream=r.handle, reads_back=True))
            host.append(r.call(sd.last_inner_stats, reads_back=True))
            r.call(sd.rhs_set, new[me], stream=r.handle, reads_back=True)
            snap_state(me, (3,))
        return host
    return body


def test_the_new_entry_points_on_a_stream(schwz, torch_cuda):
    """band_p3 with three aggregates per subdomain: rhs_set (device pointer), rhs_aggregate, restart(keep) and
    rhs_gather, rhs_aggregate, restart(zero) of all three subdomains enqueued behind the shut gate, x~, b~, y, b and
    the coarse residual s compared with the default-stream run; then the calls that read back."""
    torch = torch_cuda
    snaps, host = rig.both(torch, _stream_body(schwz, torch), "resolve entry points")
    assert host[2] == 0 and host[3] == 0.0          # last_inner_stats after a restart: (0, 0.0)
    # after restart(zero): x~ = 0, b~ = b
    x, bt, y, b = snaps[4 * 3 + 1:4 * 3 + 1 + 4]
    assert not x.any() and not y.any() and rig.same(bt, b) and np.abs(b).max() > 0
