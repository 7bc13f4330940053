"""What a z-sweep walk workgroup does before its first and after its last step (spmv_pair.hip, "Prologue"): the
fold of the previous launch's partial sums -- alpha in the update walk, rho and beta in the fused direction walk --
taken in two parts around the window requests, and the reductions of the epilogue behind one pair of barriers.  alpha
and beta feed every row of every later iterate, so a fold that dropped, doubled or misplaced a partial sum shows in x.

The walk against the chunk-by-chunk launches (SCHWZ_CG_SWEEP=0, read per solve) on the smallest shapes that take each
path: planes of two whole chunks (256 x 4 x 12, the walk_small of cg_child.py), planes that are not whole chunks
(200 x 9 x 11: byte ids, partial last band, the RUNS = 0 instantiations), and a three-slab run whose middle slab has
both neighbours (chained overlap planes, fused check residual at the start).

What can be bit for bit and what cannot.  One CG iteration from a chunk-by-chunk start: every row sees the same
products in the same order and alpha_0 is folded from the same sums, so x and the iteration count are equal bit for
bit (as in test_z_sweep_update_launch_matches_the_gather_walk).  The residual NORM is folded from the partial sums of
other workgroups (a segment is not a chunk), i.e. the same n non-negative terms r_i^2 summed in another order: each
order's relative error is below (n - 1) 2^-53, so the squares agree to 2 (n - 1) 2^-53 and the norms to n 2^-53.
Later iterations, and a solve that starts in the walk, inherit that reordering through rho: there the two iterates
are compared as tests/test_gpu_cg.py compares the device with its references -- each may be MARGIN x dev away from the
extended-precision iterate, dev = the float64 reference's own distance from it, floored at iters x 2^-52 -- so they
are at most twice that apart; the recurred residual norms likewise, with the deviation of the references' norms."""
import numpy as np
import pytest

import hp_reference as hp

pytestmark = pytest.mark.gpu

LD = np.longdouble
MARGIN = 32.0   # tests/test_gpu_cg.py
ITERS = (2, 7, 20)
FORCE_WALK = {"SCHWZ_SPMV_PATTERN": "2", "SCHWZ_SPMV_PAIR": "2", "SCHWZ_SPMV_SWEEP": "2"}
SHAPES = {
    # name: (grid, switches at upload, generic mode)
    "walk_small": ((256, 4, 12), dict(FORCE_WALK, SCHWZ_SWEEP_T="512", SCHWZ_SWEEP_L="4"), False),
    "gen_200x9": ((200, 9, 11), FORCE_WALK, True),
}
_REFS = {}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _references(name, rp, col, val, b, x0):
    """x after ITERS updates in float64 and in extended precision, once per shape"""
    if name not in _REFS:
        out = {}
        for dt in (np.float64, LD):
            keep = {k: None for k in ITERS}
            _, hist = hp.pcg(rp, col, val, b, x0, hp.precond_jacobi(rp, col, val, dt), max(ITERS), dtype=dt, keep=keep)
            out[dt] = (keep, hist)
        _REFS[name] = out
    return _REFS[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_walk_prologue_and_epilogue_against_the_chunk_launches(schwz, oracle, torch_cuda, monkeypatch, name):
    hp.require_extended_precision()
    torch = torch_cuda
    shape, env, gen = SHAPES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SCHWZ_CG_DEFERX", "2")
    rp, col, val = oracle.laplacian3d(*shape)
    n = len(rp) - 1
    A = schwz.Csr(rp, col, val)
    assert A.format() == 3 and A.symmetric() and A.sweep_slots() > 0 and A.sweep_left_out() == 0
    assert ((shape[0] * shape[1]) % 512 != 0) == gen
    cg = schwz.Pcg(A, 1)
    rng = np.random.default_rng(16)
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)

    def solve(sweep, iters, start, rtol=0.0):
        monkeypatch.setenv("SCHWZ_CG_SWEEP", sweep)
        monkeypatch.setenv("SCHWZ_CG_SWEEPSTART", start)
        d_b, d_x = _dev(torch, b), _dev(torch, x0)
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, iters)
        return it, rn, d_x.cpu().numpy(), cg.flavour()

    # one iteration, chunk-by-chunk start: alpha_0 from the fused direction walk's partial sums, folded by the update walk
    it0, rn0, x_ref, fl0 = solve("0", 1, "0")
    it1, rn1, x_sw, fl1 = solve("1", 1, "0")
    print("%s: 1 iteration, flavours %d / %d, residual norms %.17g / %.17g (equal bits: %s)" % (name, fl0, fl1, rn0, rn1, rn0 == rn1))
    assert fl0 & 24 == 0 and fl1 & 56 == 24, (fl0, fl1)
    assert it0 == it1 == 1
    assert np.array_equal(x_ref, x_sw)
    assert abs(rn0 - rn1) <= n * 2.0 ** -53 * rn0, (rn0, rn1)
    # later iterations (beta, and alpha from sums the update walk's epilogue wrote), both starts; start = "1": the INIT
    # and FIRST forms, the virtual first and last direction
    ref = _references(name, rp, col, val, b, x0)
    for iters in ITERS:
        x_ld, x_64 = ref[LD][0][iters], ref[np.float64][0][iters]
        r_ld, r_64 = float(ref[LD][1][iters]), float(ref[np.float64][1][iters])
        scale = float(np.abs(x_ld).max())
        dev = max(float(np.abs(x_64 - x_ld).max()) / scale, iters * 2.0 ** -52)
        dev_r = max(abs(r_64 - r_ld) / r_ld, iters * 2.0 ** -52)
        it0, rn0, x_ref, _ = solve("0", iters, "0")
        assert float(np.abs(x_ref - x_ld).max()) / scale <= MARGIN * dev
        for start in ("0", "1"):
            it1, rn1, x_sw, fl = solve("1", iters, start)
            assert fl & 56 == (56 if start == "1" else 24), (start, fl)
            err_ld = float(np.abs(x_sw - x_ld).max()) / scale
            err = float(np.abs(x_sw - x_ref).max()) / scale
            print("%s: %d iterations, start %s, flavour %d: walk - chunks %.2e, walk - extended %.2e, dev %.2e; norms %.17g / %.17g, dev %.2e"
                  % (name, iters, start, fl, err, err_ld, dev, rn0, rn1, dev_r))
            assert it0 == it1 == iters
            assert err_ld <= MARGIN * dev and err <= 2.0 * MARGIN * dev, (iters, start, err, err_ld, dev)
            assert abs(rn1 - r_ld) <= MARGIN * dev_r * r_ld and abs(rn0 - rn1) <= 2.0 * MARGIN * dev_r * r_ld, (iters, start, rn0, rn1, r_ld, dev_r)
    # a stop on a tolerance: the iteration count (the state workgroup 0 of the fused direction walk advances)
    it0, _, x_ref, _ = solve("0", n, "0", 1e-9)
    for start in ("0", "1"):
        it1, _, x_sw, _ = solve("1", n, start, 1e-9)
        print("%s: rtol 1e-9, start %s: %d / %d iterations" % (name, start, it0, it1))
        assert 1 < it0 < n and abs(it0 - it1) <= 1
        assert np.abs(x_ref - x_sw).max() <= 1e-8 * np.abs(x_ref).max()


def test_walk_prologue_in_a_three_slab_run(schwz, oracle, torch_cuda, monkeypatch):
    """256 x 4 x 36 in three z slabs, overlap 2, eight CG iterations per local solve, five outer iterations, all in
    one process: the middle slab's local matrix chains two appended overlap planes to its interior and its solves
    start with the fused check residual (the DUAL form of the start walk plus the listed launch of the flagged
    planes).  Walk against SCHWZ_CG_SWEEP=0: the same iteration count; solution and the residual history of every
    subdomain to 1e-8 of the CPU oracle each (the bound of smoke()), hence to 2e-8 of each other."""
    torch = torch_cuda
    shape, P = (256, 4, 36), 3
    for k, v in dict(FORCE_WALK, SCHWZ_SWEEP_T="512", SCHWZ_SWEEP_L="4", SCHWZ_CG_DEFERX="2").items():
        monkeypatch.setenv(k, v)

    def run(sweep):
        monkeypatch.setenv("SCHWZ_CG_SWEEP", sweep)
        s = schwz.Settings(laplacian_dim=3, laplacian_shape=shape)
        m = schwz.Metadata(num_subdomains=P, tolerance=1e-30, max_iters=5, local_precond="block-jacobi",
                           precond_max_block_size=1, local_solver_tolerance=0.0, local_max_iters=8)
        solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
        solver.initialize()
        out = solver.run()
        torch.cuda.synchronize()
        hist = np.asarray(m.post_process_data["global_residual_vector_out"], dtype=np.float64)
        return out, hist, [solver.subdomains[me].cg_flavour() for me in sorted(solver.subdomains)]

    out0, h0, fl0 = run("0")
    out1, h1, fl1 = run("1")
    print("three slabs: flavours %s / %s, iterations %d / %d, final residual %.17g / %.17g"
          % (fl0, fl1, out0["iter_count"], out1["iter_count"], out0["residual_norm"], out1["residual_norm"]))
    assert all(f & 24 == 0 for f in fl0) and all(f & 24 == 24 for f in fl1), (fl0, fl1)
    assert out0["iter_count"] == out1["iter_count"] == 5
    rp, col, val = oracle.laplacian3d(*shape)
    N = len(rp) - 1
    r = oracle.ras_run(rp, col, val, np.ones(N), P, oracle.first_rows_regular(N, P),
                       oracle.make_settings(max_iters=5, tol=1e-30, precond=oracle.PRECOND_JACOBI, local_tol=0.0,
                                            local_max_iters=8))
    scale = np.abs(r["solution"]).max()
    for out in (out0, out1):
        assert np.abs(out["solution"] - r["solution"]).max() <= 1e-8 * scale
    assert np.abs(out0["solution"] - out1["solution"]).max() <= 2e-8 * scale
    assert h0.shape == h1.shape and h0.size > 0
    assert np.abs(h0 - h1).max() <= 2e-8 * np.abs(h0).max()
