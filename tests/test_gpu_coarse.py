"""Two-level RAS on the GPU: the aggregation coarse correction x <- x + Z A0^-1 Z^T (b - A x) ahead of every RAS step
(Metadata.coarse_space = "aggregates", csrc/coarse.hip, schwz_ras_coarse_apply).

The reference is a float64 numpy / scipy restatement of the two-level iteration written here (class TwoLevel).  It
takes every subdomain's index sets from the library itself -- Subdomain.local_to_global and the sizes -- so it restates
no overlap rule; aggregates come from coarse_aggregate_vector.  Bounds:
  * orthogonality, right after the apply: |s_a| <= 1e-10 (|beta_a| + sum_j |W_aj x~_j|), the project's step-state
    tolerance (test_step_by_step_state_matches_oracle), far above n_c cond(A0) eps ~ 1e-13;
  * step state (x~ on all slots, b~, rho): 1e-10 relative to the largest entry, like that test;
  * whole runs: the first 6 entries of the global residual history within 1e-10 G0 of the restatement (same-algorithm
    runs are held to 1e-11 G0; the factor is cond(A0), 14 at most here), the iteration count within 1;
  * fixed inner work (CG(10)): what test_ras_3d_fixed_inner_work_matches_oracle asks -- first 6 entries to 1e-11 G0,
    the rest to 2 tol G0, the count within 2 -- and the two homes of y against each other to 1e-12 G0 over 8 steps."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import stream_rig as rig

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "schwarz-lib_amd")


# ---- inputs ------------------------------------------------------------------------------------------------------

def boxes(shape, box):
    """Aggregate id per row of an nx x ny x nz grid in natural ordering: boxes of bx x by x bz cells, numbered z-layer
    of boxes after z-layer."""
    (nx, ny, nz), (bx, by, bz) = shape, box
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    cx, cy = -(-nx // bx), -(-ny // by)
    ids = ((z // bz) * cy + y // by) * cx + x // bx
    return np.ascontiguousarray(ids.transpose(2, 1, 0).reshape(-1)).astype(np.int64)


def csr_of(rp, col, val):
    import scipy.sparse as sp
    n = len(rp) - 1
    return sp.csr_matrix((np.asarray(val, dtype=np.float64), np.asarray(col), np.asarray(rp)), shape=(n, n))


def dev_read(schwz, torch, ptr, n):
    out = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    idx = torch.arange(max(n, 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if n:
        schwz.gather(n, idx.data_ptr(), ptr, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()[:n]


# ---- the restatement ---------------------------------------------------------------------------------------------

class TwoLevel:
    """The RAS iteration of SolverRAS.step() on the host, with (agg given) or without the coarse correction.
    parts: [(local_to_global, local_size, local_size_x)] per subdomain, from the library.  local: "direct" or
    ("cg", K) for K iterations of Jacobi-preconditioned CG warm-started from y."""

    def __init__(self, A, b, parts, agg=None, local="direct"):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        self.A, self.b, self.local, self.agg = A.tocsr(), np.asarray(b, dtype=np.float64), local, agg
        self.N = A.shape[0]
        self.sub = []
        for l2g, n_int, nx in parts:
            l2g = np.asarray(l2g, dtype=np.int64)
            rows = self.A[l2g[:nx], :].tocsr()
            a_loc = rows[:, l2g[:nx]].tocsc()
            d = dict(l2g=l2g, n_int=int(n_int), nx=int(nx), rows=rows, a_loc=a_loc.tocsr(), b_loc=self.b[l2g[:nx]],
                     xt=np.zeros(len(l2g)), y=np.zeros(nx), bt=self.b[l2g[:nx]].copy(), rho=0.0)
            if nx:
                d["lu"] = spla.splu(a_loc) if local == "direct" else None
                d["dinv"] = 1.0 / a_loc.diagonal()
            self.sub.append(d)
        if agg is not None:
            nc = int(agg.max()) + 1
            self.Z = sp.csr_matrix((np.ones(self.N), (np.arange(self.N), agg)), shape=(self.N, nc))
            self.A0 = (self.Z.T @ self.A @ self.Z).toarray()
            self.A0inv = np.linalg.inv(self.A0)
        self.hist, self.g0, self.iters, self.converged = [], None, 0, False

    def global_x(self):
        x = np.zeros(self.N)
        for d in self.sub:
            x[d["l2g"][:d["n_int"]]] = d["xt"][:d["n_int"]]
        return x

    def exchange_and_correct(self):
        x = self.global_x()
        for d in self.sub:
            d["xt"][d["n_int"]:] = x[d["l2g"][d["n_int"]:]]
        if self.agg is not None:
            c = self.A0inv @ (self.Z.T @ (self.b - self.A @ x))
            for d in self.sub:
                d["xt"] += c[self.agg[d["l2g"]]]
                d["y"] += c[self.agg[d["l2g"][:d["nx"]]]]

    def boundary_and_check(self):
        total = 0.0
        for d in self.sub:
            nx = d["nx"]
            xe = np.zeros(self.N)
            xe[d["l2g"]] = d["xt"]
            loc = d["a_loc"] @ d["xt"][:nx]
            d["bt"] = d["b_loc"] - (d["rows"] @ xe - loc)
            d["rho"] = float(np.linalg.norm(d["bt"] - loc))
            total += d["rho"]
        return total

    def solve_and_restrict(self):
        for d in self.sub:
            if not d["nx"]:
                continue
            if self.local == "direct":
                d["y"] = d["lu"].solve(d["bt"])
            else:
                a, y, dinv = d["a_loc"], d["y"].copy(), d["dinv"]
                r = d["bt"] - a @ y
                z = dinv * r
                p, rho = z.copy(), float(r @ z)
                for _ in range(self.local[1]):
                    q = a @ p
                    alpha = rho / float(p @ q)
                    y += alpha * p
                    r -= alpha * q
                    z = dinv * r
                    rho, old = float(r @ z), rho
                    p = z + (rho / old) * p
                d["y"] = y
            d["xt"][:d["n_int"]] = d["y"][:d["n_int"]]

    def step(self, tol):
        self.exchange_and_correct()
        g = self.boundary_and_check()
        self.hist.append(g)
        if self.g0 is None:
            self.g0 = g
        if tol > 0.0 and g / self.g0 <= tol:
            self.converged = True
            return True
        self.solve_and_restrict()
        self.iters += 1
        return False

    def run(self, tol, max_iters):
        while self.iters < max_iters and not self.step(tol):
            pass
        return self


def parts_of(solver):
    return [(sd.local_to_global, sd.local_size, sd.local_size_x) for _, sd in sorted(solver.subdomains.items())]


def make_solver(schwz, P, settings_kw, metadata_kw, matrix=None):
    s = schwz.Settings(**settings_kw)
    m = schwz.Metadata(num_subdomains=P, **metadata_kw)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize(matrix=matrix)
    return solver, m


def history(m):
    return np.array(m.post_process_data["global_residual_vector_out"]).sum(axis=0)


# ---- 1 / 5: orthogonality ------------------------------------------------------------------------------------------

def coarse_scales(solver, torch, schwz):
    """Per subdomain |beta_a| + sum_j |W_aj x~_j| of its own aggregates, from the library's local matrix and the
    current x~ (b = 1: beta_a is the size of the aggregate)."""
    import scipy.sparse as sp
    co = solver._coarse
    agg_global = np.concatenate([co["interior"][me] for me in sorted(solver.subdomains)])
    out = {}
    for me, sd in sorted(solver.subdomains.items()):
        n, nx = sd.local_size, sd.local_size_x
        first, m = int(co["first"][me]), int(co["first"][me + 1] - co["first"][me])
        if n == 0:
            out[me] = np.zeros(0)
            continue
        rp, col, val = sd.local_matrix()
        a_int = sp.csr_matrix((val[:rp[n]], col[:rp[n]], rp[:n + 1]), shape=(n, nx))
        zt = sp.csr_matrix((np.ones(n), (agg_global[sd.local_to_global[:n]] - first, np.arange(n))), shape=(m, n))
        w = (zt @ a_int).tocsr()
        p, cnt = sd.vector(0)
        xt = dev_read(schwz, torch, p, cnt)
        out[me] = np.asarray(zt.sum(axis=1)).ravel() + abs(w) @ np.abs(xt[:nx])
    return out


def watch_orthogonality(solver, torch, schwz, steps=3):
    """Wraps the solver's coarse step: in each of the first `steps` outer steps the coarse residual is computed again
    right after the apply and compared with its scale.  Returns the list of worst ratios |s_a| / scale_a."""
    inner, seen = solver._coarse_step, []

    def wrapped(locals_, stream):
        inner(locals_, stream)
        if len(seen) >= steps:
            return
        obj = solver._coarse["obj"]
        for _, sd in locals_:
            sd.coarse_residual(obj, stream)
        s = dev_read(schwz, torch, *obj.vector(0))
        scales = coarse_scales(solver, torch, schwz)
        worst = 0.0
        for me in sorted(solver.subdomains):
            first, end = int(solver._coarse["first"][me]), int(solver._coarse["first"][me + 1])
            if end > first:
                worst = max(worst, float((np.abs(s[first:end]) / scales[me]).max()))
        seen.append(worst)
    solver._coarse_step = wrapped
    return seen


@pytest.mark.parametrize("box,nc", [((4, 4, 2), 54), ((4, 4, 4), 27)])
def test_coarse_residual_vanishes_after_the_correction_laplacian(schwz, torch_cuda, box, nc):
    """(4, 4, 4): 27 aggregates, 9 per slab -- the whole chain (residual, dense_inverse, GEMV, apply) with an odd nc."""
    shape, P = (12, 12, 12), 3
    agg = boxes(shape, box)
    solver, m = make_solver(schwz, P, dict(laplacian_dim=3, laplacian_shape=shape, local_solver="direct-ginkgo"),
                            dict(tolerance=1e-8, max_iters=200, coarse_space="aggregates", coarse_aggregate_vector=agg))
    assert solver._coarse["nc"] == nc
    seen = watch_orthogonality(solver, torch_cuda, schwz)
    out = solver.run()
    print("worst |s_a| / scale in the first steps:", seen)
    assert len(seen) == 3 and max(seen) <= 1e-10
    assert out["converged"]


def test_coarse_residual_vanishes_with_automatic_aggregates_on_ani4(schwz, torch_cuda, tmp_path):
    """ani4_crop, graph partition, 4 subdomains, 8 automatic aggregates per subdomain.  No iteration-count claim on
    this matrix: arbitrary aggregates of an anisotropic problem helped in some runs and hurt in others."""
    g = np.load(os.path.join(G, "ani4_crop.npz"))
    n = len(g["rp"]) - 1
    solver, m = make_solver(schwz, 4, dict(explicit_laplacian=False, partition=schwz.PARTITION_METIS,
                                           local_solver="direct-ginkgo"),
                            dict(tolerance=1e-8, max_iters=3000, coarse_space="aggregates", coarse_aggregates=8),
                            matrix=(g["rp"].astype(np.int64), g["col"], g["val"]))
    co = solver._coarse
    assert co["nc"] <= 32
    seen_ids = []
    for me, sd in sorted(solver.subdomains.items()):
        ids = co["interior"][me]
        assert len(ids) == sd.local_size                     # every interior row has exactly one aggregate ...
        assert ids.min() >= co["first"][me] and ids.max() < co["first"][me + 1]   # ... of its own subdomain
        assert len(np.unique(ids)) == co["first"][me + 1] - co["first"][me]      # ... and no aggregate is empty
        seen_ids.append(ids)
    assert sum(len(i) for i in seen_ids) == n
    seen = watch_orthogonality(solver, torch_cuda, schwz)
    out = solver.run()
    print("ani4_crop: %d outer iterations, worst |s_a| / scale %s" % (out["iter_count"], seen))
    assert len(seen) == 3 and max(seen) <= 1e-10
    assert out["converged"]


@pytest.mark.parametrize("local", ["gmres", "umfpack"])
def test_coarse_correction_of_a_non_symmetric_matrix(schwz, torch_cuda, convdiff, local):
    rp, col, val = convdiff(12)
    agg = np.arange(144) // 8            # 48 rows per subdomain: 6 aggregates of 8 consecutive rows each
    skw = dict(explicit_laplacian=False, non_symmetric_matrix=True)
    if local == "umfpack":
        skw.update(local_solver="direct-ginkgo", factorization="umfpack")
    else:
        skw.update(restart_iter=10)
    solver, m = make_solver(schwz, 3, skw, dict(tolerance=1e-8, max_iters=400, coarse_space="aggregates",
                                               coarse_aggregate_vector=agg),
                            matrix=(rp.astype(np.int64), col, val))
    a0 = np.vstack([sd.coarse_rows() for _, sd in sorted(solver.subdomains.items())])
    assert np.abs(a0 - a0.T).max() > 0.1                    # A0 is non-symmetric: the LU, not a Cholesky, inverts it
    seen = watch_orthogonality(solver, torch_cuda, schwz)
    out = solver.run()
    print("convdiff %s: %d outer iterations, worst |s_a| / scale %s" % (local, out["iter_count"], seen))
    assert len(seen) == 3 and max(seen) <= 1e-10
    assert out["converged"]
    x = csr_of(rp, col, val)
    assert np.linalg.norm(np.ones(144) - x @ out["solution"]) <= 1e-6 * 12.0


# ---- 2: step-by-step state -----------------------------------------------------------------------------------------

def test_step_by_step_state_matches_the_restatement(schwz, torch_cuda):
    """Drives the C-ABI steps by hand for 3 outer iterations -- pack, exchange, unpack, coarse residual, solve, apply,
    boundary update, check, local solve, restriction -- and compares x~ on all slots after the apply, b~ and rho."""
    torch = torch_cuda
    shape, P = (12, 12, 12), 3
    N = shape[0] * shape[1] * shape[2]
    agg = boxes(shape, (4, 4, 2))
    prob = schwz.Problem.laplacian(3, *shape)
    A = csr_of(*prob.to_csr())
    fr = schwz.partition_regular(N, P)
    sds = [schwz.Subdomain(prob, P, me, 2, fr) for me in range(P)]
    for me, lst in schwz.InProcessComm(P).handshake({me: sd.get_lists() for me, sd in enumerate(sds)}).items():
        for q, ids in lst:
            sds[me].add_put_list(q, ids)
    send, recv = [], []
    for sd in sds:
        sd.to_device(np.ones(sd.local_size_x), local_solver=schwz.capi.SOLVER_DIRECT)
        send.append(torch.zeros(max(sd.num_send, 1), dtype=torch.float64, device="cuda"))
        recv.append(torch.zeros(max(sd.num_recv, 1), dtype=torch.float64, device="cuda"))
    first = [0, 18, 36, 54]
    for me, sd in enumerate(sds):
        own = agg[sd.local_to_global[:sd.local_size]]
        assert own.min() == first[me] and own.max() == first[me + 1] - 1
        sd.coarse_set_aggregates(agg[sd.local_to_global], first[me], 18, 54)
    a0 = np.vstack([sd.coarse_rows() for sd in sds])
    ref = TwoLevel(A, np.ones(N), [(sd.local_to_global, sd.local_size, sd.local_size_x) for sd in sds], agg)
    assert np.abs(a0 - ref.A0).max() <= 1e-13 * np.abs(ref.A0).max()
    coarse = schwz.Coarse(schwz.dense_inverse(a0))

    def close(got, want, what):
        err = np.abs(got - want).max() / (np.abs(want).max() + 1e-300)
        print("%s: %.2e" % (what, err))
        assert err <= 1e-10, what

    for it in range(3):
        bufs = {}
        for me, sd in enumerate(sds):
            sd.pack(send[me].data_ptr())
            off = sd.send_offsets()
            for k, (q, _) in enumerate(sd.put_lists()):
                bufs[(me, q)] = send[me][off[k]:off[k + 1]]
        for me, sd in enumerate(sds):
            off = sd.recv_offsets()
            for k, (p, _) in enumerate(sd.get_lists()):
                recv[me][off[k]:off[k + 1]].copy_(bufs[(p, me)])
            sd.unpack(recv[me].data_ptr())
        for sd in sds:
            sd.coarse_residual(coarse)
        coarse.solve()
        for sd in sds:
            sd.coarse_apply(coarse)
        ref.exchange_and_correct()
        for me, sd in enumerate(sds):
            close(dev_read(schwz, torch, *sd.vector(0)), ref.sub[me]["xt"], "step %d subdomain %d x~" % (it, me))
        ref.boundary_and_check()
        for me, sd in enumerate(sds):
            sd.update_boundary()
            close(dev_read(schwz, torch, *sd.vector(1)), ref.sub[me]["bt"], "step %d subdomain %d b~" % (it, me))
            rho = sd.local_residual()
            scale = np.abs(ref.sub[me]["bt"]).max()
            print("step %d subdomain %d rho: %.3e against %.3e" % (it, me, rho, ref.sub[me]["rho"]))
            assert abs(rho - ref.sub[me]["rho"]) <= 1e-10 * max(scale, ref.sub[me]["rho"])
            sd.local_solve()
            sd.restrict()
        ref.solve_and_restrict()
    torch.cuda.synchronize()


# ---- 3: whole run, and the point of the feature ----------------------------------------------------------------------

def test_two_level_run_matches_the_restatement_and_needs_fewer_iterations(schwz, torch_cuda):
    shape, P, tol = (16, 16, 64), 8, 1e-8
    N = shape[0] * shape[1] * shape[2]
    agg = boxes(shape, (4, 4, 4))
    skw = dict(laplacian_dim=3, laplacian_shape=shape, local_solver="direct-ginkgo", overlap=2)
    two, m2 = make_solver(schwz, P, skw, dict(tolerance=tol, max_iters=200, coarse_space="aggregates",
                                              coarse_aggregate_vector=agg))
    assert two._coarse["nc"] == 256
    out2 = two.run()
    one, m1 = make_solver(schwz, P, skw, dict(tolerance=tol, max_iters=200))
    out1 = one.run()
    A = csr_of(*two.problem.to_csr())
    ref2 = TwoLevel(A, np.ones(N), parts_of(two), agg).run(tol, 200)
    ref1 = TwoLevel(A, np.ones(N), parts_of(one)).run(tol, 200)
    h2 = history(m2)
    g0 = ref2.hist[0]
    print("outer iterations: device %d -> %d, restatement %d -> %d" %
          (out1["iter_count"], out2["iter_count"], ref1.iters, ref2.iters))
    print("history, first 6 entries, |device - restatement| / G0:", np.abs(h2[:6] - np.array(ref2.hist[:6])) / g0)
    assert out1["converged"] and out2["converged"] and ref1.converged and ref2.converged
    assert np.abs(h2[:6] - np.array(ref2.hist[:6])).max() <= 1e-10 * g0
    assert abs(out2["iter_count"] - ref2.iters) <= 1
    assert ref2.iters < ref1.iters
    assert out2["iter_count"] < out1["iter_count"]
    # the one-level run is today's: the restatement without the correction is its reference too
    assert abs(out1["iter_count"] - ref1.iters) <= 1
    x = np.linalg.norm(np.ones(N) - A @ out2["solution"])
    assert x <= 1e-6 * np.sqrt(N)


# ---- 4: both homes of y --------------------------------------------------------------------------------------------

def test_the_warm_start_moves_with_the_correction_in_both_homes_of_y(schwz, torch_cuda, monkeypatch):
    """One subdomain, CG + Jacobi with exactly 10 inner iterations.  SCHWZ_CG_DEFERX=2: y lives in the x~ buffers
    (the apply pass adds once); SCHWZ_CG_DEFERX=0: y is a buffer of its own (the apply launch adds to both)."""
    shape, tol = (16, 10, 7), 1e-10   # (9 history entries; at 1e-8 the run ends after 7, and 8 are compared)
    N = shape[0] * shape[1] * shape[2]
    agg = boxes(shape, (4, 5, 4))
    runs = {}
    for deferx in ("2", "0"):
        monkeypatch.setenv("SCHWZ_CG_DEFERX", deferx)
        solver, m = make_solver(schwz, 1, dict(laplacian_dim=3, laplacian_shape=shape),
                                dict(tolerance=tol, max_iters=200, local_precond="block-jacobi", precond_max_block_size=1,
                                     local_solver_tolerance=0.0, local_max_iters=10, coarse_space="aggregates",
                                     coarse_aggregate_vector=agg))
        sd = solver.subdomains[0]
        forms = [sd.y_form()]
        solver.begin_run()
        while m.iter_count < m.max_iters:
            if solver.step():
                break
            forms.append(sd.y_form())
        out = solver.finish_run(0.0)
        if deferx == "2":
            assert all(f != 0 for f in forms), forms
        else:
            assert all(f == 0 for f in forms), forms
        runs[deferx] = (out, history(m), solver)
    A = csr_of(*runs["2"][2].problem.to_csr())
    ref = TwoLevel(A, np.ones(N), parts_of(runs["2"][2]), agg, local=("cg", 10)).run(tol, 200)
    g0 = ref.hist[0]
    for deferx, (out, h, _) in runs.items():
        k = min(len(h), len(ref.hist))
        print("SCHWZ_CG_DEFERX=%s: %d iterations (restatement %d), first 6 |diff| / G0 %s" %
              (deferx, out["iter_count"], ref.iters, np.abs(h[:6] - np.array(ref.hist[:6])) / g0))
        assert out["converged"] and abs(out["iter_count"] - ref.iters) <= 2
        assert np.abs(h[:6] - np.array(ref.hist[:6])).max() <= 1e-11 * g0
        assert np.abs(h[:k] - np.array(ref.hist[:k])).max() <= 2.0 * tol * g0
    ha, hb = runs["2"][1], runs["0"][1]
    print("the two homes of y against each other, 8 steps, / G0:", np.abs(ha[:8] - hb[:8]) / g0)
    assert len(ha) >= 8 and len(hb) >= 8
    assert np.abs(ha[:8] - hb[:8]).max() <= 1e-12 * g0


# ---- 6: several processes --------------------------------------------------------------------------------------------

_RANK = """
import json, os, sys
sys.path.insert(0, %(pkg)r)
import numpy as np
import torch
import torch.distributed as dist
import schwz_amd as S
dist.init_process_group("gloo")
torch.cuda.set_device(0)
comm = S.TorchDistComm(device=torch.device("cuda", 0))
agg = np.load(%(agg)r)
s = S.Settings(laplacian_dim=3, laplacian_shape=(12, 12, 12), local_solver="direct-ginkgo")
m = S.Metadata(tolerance=1e-8, max_iters=200, coarse_space="aggregates", coarse_aggregate_vector=agg)
solver = S.SolverRAS(s, m, comm=comm, quiet=True)
solver.initialize()
out = solver.run()
hist = np.array(m.post_process_data["global_residual_vector_out"]).sum(axis=0)
if comm.rank == 0:
    np.save(%(sol)r, out["solution"])
    np.save(%(hist)r, hist)
print(json.dumps(dict(rank=comm.rank, iters=out["iter_count"], conv=bool(out["converged"]))), flush=True)
dist.destroy_process_group()
"""


def test_three_rank_processes_match_the_in_process_run(schwz, torch_cuda, tmp_path):
    """Three rank processes share this GPU over gloo: the segments of s are all-gathered through the host, every rank
    inverts the same A0.  History and solution equal the in-process run to 1e-12 relative."""
    import json
    shape, world = (12, 12, 12), 3
    agg = boxes(shape, (4, 4, 2))
    np.save(str(tmp_path / "agg.npy"), agg)
    sol, hist = str(tmp_path / "sol.npy"), str(tmp_path / "hist.npy")
    script = tmp_path / "rank.py"
    script.write_text(_RANK % dict(pkg=PKG, agg=str(tmp_path / "agg.npy"), sol=sol, hist=hist))
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            o, e = p.communicate()
        assert p.returncode == 0, o + e[-3000:]
        outs.append(json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]))
    assert all(o["conv"] for o in outs) and len({o["iters"] for o in outs}) == 1
    solver, m = make_solver(schwz, world, dict(laplacian_dim=3, laplacian_shape=shape, local_solver="direct-ginkgo"),
                            dict(tolerance=1e-8, max_iters=200, coarse_space="aggregates", coarse_aggregate_vector=agg))
    out = solver.run()
    assert out["converged"] and out["iter_count"] == outs[0]["iters"]
    got, h = np.load(sol), np.load(hist)
    assert np.abs(got - out["solution"]).max() <= 1e-12 * np.abs(out["solution"]).max()
    assert len(h) == len(history(m)) and np.abs(h - history(m)).max() <= 1e-12 * history(m)[0]


# ---- 7: streams ------------------------------------------------------------------------------------------------------

def test_coarse_entry_points_obey_their_stream(schwz, torch_cuda):
    """schwz_ras_coarse_residual, schwz_coarse_solve and schwz_ras_coarse_apply on a non-default stream held shut by a
    delay, beside a default stream that runs: every call returns while the gate is shut, and x~, y, s and c equal the
    default-stream run bit for bit (stream_rig.py: a launch on another stream reads poison or is overwritten)."""
    torch = torch_cuda
    shape, P = (12, 12, 12), 3
    N = shape[0] * shape[1] * shape[2]
    agg = boxes(shape, (4, 4, 2))
    first = [0, 18, 36, 54]

    def body(r):
        prob = r.hold(schwz.Problem.laplacian(3, *shape))
        fr = schwz.partition_regular(N, P)
        sds = [r.hold(schwz.Subdomain(prob, P, me, 2, fr)) for me in range(P)]
        idx, true_x, true_y = [], [], []
        for me, sd in enumerate(sds):
            sd.to_device(np.ones(sd.local_size_x), precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=4)
            sd.coarse_set_aggregates(agg[sd.local_to_global], first[me], 18, 54)
            nx = sd.local_size_x + sd.halo_size
            idx.append(r.hold(torch.arange(nx, dtype=torch.int32, device="cuda")))
            rng = np.random.default_rng(70 + me)
            true_x.append(r.hold(torch.from_numpy(rng.standard_normal(nx)).cuda()))
            true_y.append(r.hold(torch.from_numpy(rng.standard_normal(sd.local_size_x)).cuda()))
            assert sd.y_form() == 0
        coarse = r.hold(schwz.Coarse(schwz.dense_inverse(np.vstack([sd.coarse_rows() for sd in sds]))))
        poison = r.hold(torch.full((N,), float("nan"), dtype=torch.float64, device="cuda"))
        for me, sd in enumerate(sds):
            for which, true in ((0, true_x[me]), (2, true_y[me])):
                p, cnt = sd.vector(which)
                schwz.gather(cnt, idx[me].data_ptr(), (poison if r.gated else true).data_ptr(), p)
        r.arm()
        if r.gated:                                           # behind the gate: x~ and y take their true values
            for me, sd in enumerate(sds):
                for which, true in ((0, true_x[me]), (2, true_y[me])):
                    p, cnt = sd.vector(which)
                    schwz.gather(cnt, idx[me].data_ptr(), true.data_ptr(), p, stream=r.handle)
        for sd in sds:
            r.call(sd.coarse_residual, coarse, stream=r.handle)
        r.call(coarse.solve, stream=r.handle)
        for sd in sds:
            r.call(sd.coarse_apply, coarse, stream=r.handle)
        for which in (0, 1):
            p, cnt = coarse.vector(which)
            t = r.output(cnt)
            schwz.gather(cnt, idx[0].data_ptr(), p, t.data_ptr(), stream=r.handle)
            r.snap(t)
        for me, sd in enumerate(sds):
            for which in (0, 2):
                p, cnt = sd.vector(which)
                t = r.output(cnt)
                schwz.gather(cnt, idx[me].data_ptr(), p, t.data_ptr(), stream=r.handle)
                r.snap(t)
        return []

    snaps, _ = rig.both(torch, body, "coarse step")
    s, c = snaps[0], snaps[1]
    assert np.isfinite(s).all() and np.abs(c).max() > 0
    for me in range(P):
        assert np.isfinite(snaps[2 + 2 * me]).all() and np.isfinite(snaps[3 + 2 * me]).all()
