"""SolverRAS.solve_many and the block forms of the RAS step kernels (csrc/batch.hip) against the CPU oracle, column by
column, at the bounds of tests/test_gpu_ras.py (imported, not copied).

Matrix and partition follow tests/test_gpu_resolve.py: lap3d_16x10x7 (1120 rows), overlap 2, on one subdomain and on
three with first_row = [0, 30, 575, 1120] -- local sizes 76 (one workgroup, below a tile), 735 and 705 (odd, several
tiles).  Jacobi, tolerance 1e-8, at most 300 outer iterations.  Five columns: one block of 8 with three padding columns.
With the CPU oracle, for three subdomains, every column converges, after 18, 16, 14, 16, 17 outer iterations with
converged local solves and after 18, 16, 14, 15, 17 with 10 fixed inner iterations; the stopping ratios lie at least
5 % from the tolerance on either side, and the counts differ between columns, so the freeze mask is exercised."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import stream_rig as rig
import test_gpu_ras as tras

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "schwarz-lib_amd")
LAP = (16, 10, 7)
N = 16 * 10 * 7
FR3 = np.array([0, 30, 575, N], dtype=np.int64)
CONVERGED = dict(local_solver_tolerance=1e-10)
FIXED10 = dict(local_solver_tolerance=0.0, local_max_iters=10)


def columns(n=5):
    rng = np.random.default_rng(7)
    cols = [np.ones(N), rng.standard_normal(N), rng.standard_normal(N) * 2.0 ** 20, rng.standard_normal(N) * 2.0 ** -20,
            np.sin(0.01 * np.arange(N))]
    cols += [rng.standard_normal(N) * 10.0 ** k for k in (1, -1, 3, 0)]      # beyond the five: for the block boundaries
    return np.ascontiguousarray(np.stack(cols[:n], axis=1))


def make_solver(schwz, P, inner):
    kw = dict(laplacian_dim=3, laplacian_shape=LAP)
    if P == 3:
        part = np.searchsorted(FR3, np.arange(N), side="right") - 1
        kw.update(partition=schwz.PARTITION_CUSTOM, partition_vector=part)
    s = schwz.Settings(**kw)
    m = schwz.Metadata(num_subdomains=P, tolerance=1e-8, max_iters=300, local_precond="block-jacobi",
                       precond_max_block_size=1, **inner)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize()
    if P == 3:
        assert list(m.first_row) == list(FR3)
        assert [sd.local_size_x for sd in solver.subdomains.values()] == [76, 735, 705]
        assert m.permutation is None or np.array_equal(m.permutation, np.arange(N))
    return solver, m


_runs = {}


def block_run(schwz, oracle, P, kind):
    """solve_many of the five columns and the oracle's run per column: computed once per (P, kind), never written to."""
    if (P, kind) not in _runs:
        solver, m = make_solver(schwz, P, CONVERGED if kind == "converged" else FIXED10)
        B = columns()
        out = solver.solve_many(B)
        rp, col, val = oracle.laplacian3d(*LAP)
        fr = np.asarray(m.first_row, dtype=np.int32)
        refs = [oracle.ras_run(rp, col, val, B[:, j], P, fr, tras._oracle_settings(oracle, m, solver.settings))
                for j in range(B.shape[1])]
        _runs[P, kind] = (solver, m, B, out, refs)
    return _runs[P, kind]


# ---- the step kernels ----------------------------------------------------------------------------------------------------

def _read(schwz, torch, ptr, n):
    idx = torch.arange(max(n, 1), dtype=torch.int32, device="cuda")
    t = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    schwz.gather(n, idx.data_ptr(), ptr, t.data_ptr())
    torch.cuda.synchronize()
    return t.cpu().numpy()[:n]


@pytest.mark.parametrize("K", [2, 4, 8])
def test_one_hand_driven_step_matches_the_oracle_state(schwz, oracle, torch_cuda, K):
    """Two outer steps by hand -- pack, exchange through InProcessComm, unpack, boundary update, residual, local solve,
    restriction -- on three subdomains: every column of b~ and every local norm against the oracle's state of that
    column at 1e-10 relative (the bound of test_gpu_ras.test_step_by_step_state_matches_oracle), and column j of the
    send buffer equal to the single-vector pack of that column, bit for bit."""
    torch = torch_cuda
    P = 3
    prob = schwz.Problem.laplacian(3, *LAP)
    rp, col, val = oracle.laplacian3d(*LAP)
    B = columns(8)[:, :K]
    sds = [schwz.Subdomain(prob, P, me, 2, FR3) for me in range(P)]
    osds = [oracle.Subdomain(rp, col, val, P, me, 2, FR3.astype(np.int32)) for me in range(P)]
    oracle.connect(osds)
    comm = schwz.InProcessComm(P)
    for me, lst in comm.handshake({me: sd.get_lists() for me, sd in enumerate(sds)}).items():
        for q, ids in lst:
            sds[me].add_put_list(q, ids)
    os_ = oracle.make_settings(precond=1, local_tol=0.0, local_max_iters=6)
    sts = [[oracle.State(osd, B[:, j], os_) for osd in osds] for j in range(K)]
    send, recv, single = [], [], []
    for sd in sds:
        l2g = sd.local_to_global[:sd.local_size_x]
        sd.to_device(np.ones(sd.local_size_x), precond=1, local_tol=0.0, local_max_iters=6)
        sd.batch_begin(K)
        sd.batch_rhs_set(B[l2g])
        send.append(torch.zeros(max(sd.num_send, 1) * K, dtype=torch.float64, device="cuda"))
        recv.append(torch.zeros(max(sd.num_recv, 1) * K, dtype=torch.float64, device="cuda"))
        single.append(torch.zeros(max(sd.num_send, 1), dtype=torch.float64, device="cuda"))
    for it in range(2):
        sends, recvs = {}, {}
        for me, sd in enumerate(sds):
            sd.batch_pack(send[me].data_ptr())
            torch.cuda.synchronize()
            packed = send[me].cpu().numpy()[:sd.num_send * K].reshape(sd.num_send, K)
            # the single-vector pack of column j: x~ of the single-vector state takes the block's column, then pack
            p0, n0 = sd.vector(0)
            pb, nb = sd.batch_vector(0)
            assert nb == n0 * K
            xb = _read(schwz, torch, pb, nb).reshape(n0, K)
            for j in range(K):
                t = torch.from_numpy(np.ascontiguousarray(xb[:, j])).cuda()
                idx = torch.arange(n0, dtype=torch.int32, device="cuda")
                schwz.scatter(n0, idx.data_ptr(), t.data_ptr(), p0)
                sd.pack(single[me].data_ptr())
                torch.cuda.synchronize()
                assert rig.same(np.ascontiguousarray(packed[:, j]), single[me].cpu().numpy()[:sd.num_send]), (me, j)
            off = sd.send_offsets()
            for k, (q, _) in enumerate(sd.put_lists()):
                sends[(me, q)] = send[me][off[k] * K:off[k + 1] * K]
                for j in range(K):
                    exp = sts[j][me].pack(k)
                    got = packed[off[k]:off[k + 1], j]
                    assert np.abs(got - exp).max() <= 1e-10 * (np.abs(exp).max() + 1e-300)
            off = sd.recv_offsets()
            for k, (p, _) in enumerate(sd.get_lists()):
                recvs[(p, me)] = recv[me][off[k] * K:off[k + 1] * K]
        omsgs = {(j, me, q): sts[j][me].pack(k) for j in range(K) for me in range(P)
                 for k, (q, _) in enumerate(osds[me].put_lists())}
        comm.exchange(sends, recvs)
        for me, sd in enumerate(sds):
            for j in range(K):
                for k, (p, _) in enumerate(sd.get_lists()):
                    sts[j][me].unpack(k, omsgs[(j, p, me)])
            sd.batch_unpack(recv[me].data_ptr())
            sd.batch_update_boundary()
            bt = _read(schwz, torch, *sd.batch_vector(1)).reshape(sd.local_size_x, K)
            norms = sd.batch_local_residual()
            sd.batch_local_solve(0)
            sd.batch_restrict(0)
            for j in range(K):
                st = sts[j][me]
                st.update_boundary()
                want = st.local_solution()
                assert np.abs(bt[:, j] - want).max() <= 1e-10 * (np.abs(want).max() + 1e-300), (it, me, j)
                rho = st.local_residual()
                assert abs(norms[j] - rho) <= 1e-10 * (rho + 1e-300), (it, me, j, norms[j], rho)
                st.local_solve()
                st.restrict()
    for me, sd in enumerate(sds):            # after two steps the iterates still agree
        x = _read(schwz, torch, *sd.batch_vector(0)).reshape(-1, K)[:sd.local_size]
        for j in range(K):
            want = sts[j][me].global_solution()[FR3[me]:FR3[me + 1]]
            assert np.abs(x[:, j] - want).max() <= 1e-9 * (np.abs(want).max() + 1e-300), (me, j)
    for per_column in sts:
        for st in per_column:
            st.close()


# ---- whole runs -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 3])
def test_whole_run_with_converged_local_solves(schwz, oracle, torch_cuda, P):
    """Per column against oracle.ras_run with that column as right-hand side, at the constants of
    test_gpu_ras._check_against_oracle: equal iteration count, history within TOL_HIST * G0, solution within
    TOL_SOL * max |x|, residual norm within 1e-6 * rhs norm, rhs norm within 1e-12."""
    solver, m, B, out, refs = block_run(schwz, oracle, P, "converged")
    assert out["solution"].shape == (N, 5) and len(out["iter_count"]) == 5
    if P == 3:
        assert [r["iter_count"] for r in refs] == [18, 16, 14, 16, 17]
    for j, r in enumerate(refs):
        h = np.array(out["history"][j])
        print("column %d: %d iterations (oracle %d), |hist diff| / G0 %.2e, |x diff| / max|x| %.2e" %
              (j, out["iter_count"][j], r["iter_count"], np.abs(h - r["hist_global"][:len(h)]).max() / r["hist_global"][0],
               np.abs(out["solution"][:, j] - r["solution"]).max() / np.abs(r["solution"]).max()))
        assert r["converged"] and out["converged"][j]
        assert out["iter_count"][j] == r["iter_count"]
        g0 = r["hist_global"][0]
        assert len(h) == len(r["hist_global"]) and np.abs(h - r["hist_global"]).max() <= tras.TOL_HIST * g0
        assert np.abs(out["solution"][:, j] - r["solution"]).max() <= tras.TOL_SOL * np.abs(r["solution"]).max()
        assert abs(out["residual_norm"][j] - r["residual_norm"]) <= 1e-6 * r["rhs_norm"]
        assert abs(out["rhs_norm"][j] - r["rhs_norm"]) <= 1e-12 * r["rhs_norm"]
    # the stops are away from the tolerance, and the columns stop at different iterations (the mask is exercised)
    for j, r in enumerate(refs):
        ratios = r["hist_global"] / r["hist_global"][0] / m.tolerance
        assert not ((ratios > 1 / 1.05) & (ratios < 1.05)).any(), (j, ratios[-2:])
    assert P == 1 or len(set(out["iter_count"])) > 1      # (one subdomain with a converged solve: one step each)


@pytest.mark.parametrize("P", [1, 3])
def test_whole_run_with_ten_fixed_inner_iterations(schwz, oracle, torch_cuda, P):
    """The truncated_cg rules of test_gpu_ras._check_against_oracle per column: counts within +-2, the first 6 history
    entries within 1e-11 * G0, the rest within 2 * tolerance * G0, the solution within 1e-4."""
    solver, m, B, out, refs = block_run(schwz, oracle, P, "fixed10")
    if P == 3:
        assert [r["iter_count"] for r in refs] == [18, 16, 14, 15, 17]
    for j, r in enumerate(refs):
        h = np.array(out["history"][j])
        k = min(len(h), len(r["hist_global"]))
        g0 = r["hist_global"][0]
        print("column %d: %d iterations (oracle %d), first 6 |hist diff| / G0 %.2e, all %.2e" %
              (j, out["iter_count"][j], r["iter_count"], np.abs(h[:6] - r["hist_global"][:6]).max() / g0,
               np.abs(h[:k] - r["hist_global"][:k]).max() / g0))
        assert r["converged"] and out["converged"][j]
        assert abs(out["iter_count"][j] - r["iter_count"]) <= 2
        assert np.abs(h[:6] - r["hist_global"][:6]).max() <= 1e-11 * g0
        assert np.abs(h[:k] - r["hist_global"][:k]).max() <= 2.0 * m.tolerance * g0
        assert np.abs(out["solution"][:, j] - r["solution"]).max() <= 1e-4 * np.abs(r["solution"]).max()
        assert abs(out["rhs_norm"][j] - r["rhs_norm"]) <= 1e-12 * r["rhs_norm"]


@pytest.mark.parametrize("kind", ["converged", "fixed10"])
def test_block_boundaries(schwz, oracle, torch_cuda, kind):
    """3 columns (a block of 4) and 9 columns (blocks of 8 and 2) return, for the columns they share with it, the bits
    of the 5-column run (a block of 8): nothing depends on the width of a block or on what its other columns hold."""
    solver, m, B, out, _ = block_run(schwz, oracle, 3, kind)
    for n in (3, 9):
        Bn = columns(n)
        assert rig.same(np.ascontiguousarray(Bn[:, :min(n, 5)]), np.ascontiguousarray(B[:, :min(n, 5)]))
        got = solver.solve_many(Bn)
        assert got["solution"].shape == (N, n) and len(got["iter_count"]) == n and all(got["converged"])
        for j in range(min(n, 5)):
            assert got["iter_count"][j] == out["iter_count"][j], (n, j)
            assert got["history"][j] == out["history"][j], (n, j)
            assert rig.same(np.ascontiguousarray(got["solution"][:, j]), np.ascontiguousarray(out["solution"][:, j])), (n, j)
            assert got["residual_norm"][j] == out["residual_norm"][j] and got["rhs_norm"][j] == out["rhs_norm"][j]


@pytest.mark.parametrize("P", [1, 3])
def test_single_vector_state_is_untouched(schwz, torch_cuda, P):
    """solve(b), solve_many(...), solve(b): the same iteration count, histories and solution, bit for bit."""
    solver, m = make_solver(schwz, P, FIXED10)
    B = columns()
    b = B[:, 1].copy()

    def single():
        out = solver.solve(b)
        ppd = m.post_process_data
        return (out["iter_count"], out["converged"], [list(h) for h in ppd["global_residual_vector_out"]],
                list(ppd["local_residual_vector_out"]), out["residual_norm"], out["solution"].copy())
    before = single()
    many = solver.solve_many(B)
    after = single()
    assert before[:5] == after[:5] and rig.same(before[5], after[5])
    assert all(many["converged"]) and before[1]
    # and the block run of that column is the single run's iteration, to the bounds of the oracle comparison
    assert abs(many["iter_count"][1] - before[0]) <= 2
    assert np.abs(many["solution"][:, 1] - before[5]).max() <= 1e-4 * np.abs(before[5]).max()


# ---- several processes ----------------------------------------------------------------------------------------------------

_RANK = """
import json, os, sys
sys.path.insert(0, %(pkg)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import torch
import torch.distributed as dist
import schwz_amd as S
import test_gpu_batch_ras as T
dist.init_process_group("gloo")
torch.cuda.set_device(0)
comm = S.TorchDistComm(device=torch.device("cuda", 0))
part = np.searchsorted(T.FR3, np.arange(T.N), side="right") - 1
s = S.Settings(laplacian_dim=3, laplacian_shape=T.LAP, partition=S.PARTITION_CUSTOM, partition_vector=part)
m = S.Metadata(num_subdomains=3, tolerance=1e-8, max_iters=300, local_precond="block-jacobi", precond_max_block_size=1,
               **T.FIXED10)
solver = S.SolverRAS(s, m, comm=comm, quiet=True)
solver.initialize()
out = solver.solve_many(T.columns())
if comm.rank == 0:
    np.save(%(sol)r, out["solution"])
    np.save(%(hist)r, np.array([h + [0.0] * (40 - len(h)) for h in out["history"]]))
print(json.dumps(dict(rank=comm.rank, iters=out["iter_count"], conv=[bool(c) for c in out["converged"]],
                      res=out["residual_norm"], sol=out["solution"] is not None)), flush=True)
dist.destroy_process_group()
"""


def test_three_rank_processes_match_the_in_process_run(schwz, oracle, torch_cuda, tmp_path):
    """Three rank processes share this GPU over gloo (the two-sided TorchDistComm, halos staged through the host):
    solve_many equals the in-process run bit for bit.  Fresh children, each under a timeout."""
    world = 3
    sol, hist = str(tmp_path / "sol.npy"), str(tmp_path / "hist.npy")
    script = tmp_path / "rank.py"
    script.write_text(_RANK % dict(pkg=PKG, tests=os.path.dirname(os.path.abspath(__file__)), sol=sol, hist=hist))
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
    solver, m, B, out, _ = block_run(schwz, oracle, 3, "fixed10")
    for o in outs:
        assert o["iters"] == out["iter_count"] and o["conv"] == out["converged"] and o["res"] == out["residual_norm"]
        assert o["sol"] == (o["rank"] == 0)
    got, h = np.load(sol), np.load(hist)
    assert rig.same(got, out["solution"])
    for j in range(5):
        assert list(h[j][:len(out["history"][j])]) == out["history"][j] and not h[j][len(out["history"][j]):].any()
