"""The z-sweep walks' entry (spmv_pair.hip, step 1 of the prologue): stop_iter, the slot's record -- segment and first
five chain rows --, rho, the lane sums and the table entries in their staged form are requested before anything is
waited for, the early return and the empty-slot branch follow that wait, and the tables reach LDS behind the window
requests.  A record with a wrong plane moves a whole window, a table entry that lost its value or kept one it should
not have changes every row of its pattern, and a return taken too late or not at all shows in x and in the iteration
count -- so the walk is held against the chunk-by-chunk launches (SCHWZ_CG_SWEEP=0, read per solve) on the smallest
shapes that reach each path, those of tests/test_gpu_walk_prologue.py:

  256 x 4 x 12 with SCHWZ_SWEEP_T=512 SCHWZ_SWEEP_L=4   whole-chunk planes, short segments, segments that begin at a
                                                        chain end, empty slots
  200 x 9 x 11                                          RUNS = 0: byte ids, partial last band
  256 x 4 x 36 in three slabs, overlap 2                the middle slab's local matrix: appended overlap planes chained
                                                        to the interior, a last segment of two positions whose
                                                        lookahead holds -1; in a three-slab run in one process the
                                                        DUAL form of the start walk

One CG iteration from a chunk-by-chunk start is equal bit for bit (every row sees the same products in the same order,
alpha_0 is folded from the same sums).  Later iterations and a start in the walk inherit a reordered residual norm
through rho; there both iterates are held to the extended-precision iterate as tests/test_gpu_walk_prologue.py and
tests/test_gpu_cg.py hold them: MARGIN x dev each, dev = the float64 reference's own distance from it, floored at
iters x 2^-52 -- the project's numbers, not new ones.  A start residual of exactly zero (small integers in x0, so that
b = A x0 is exact in any order) must return zero iterations with x untouched: the update walk behind the
first-direction walk, and the steady fused direction walk behind a chunk-by-chunk start, leave through the moved
return.  A stop on a tolerance reaches the chunk launches' iteration count +- 1."""
import numpy as np
import pytest

import hp_reference as hp

pytestmark = pytest.mark.gpu

LD = np.longdouble
MARGIN = 32.0   # tests/test_gpu_cg.py
ITERS = (2, 7, 20)
FORCE_WALK = {"SCHWZ_SPMV_PATTERN": "2", "SCHWZ_SPMV_PAIR": "2", "SCHWZ_SPMV_SWEEP": "2"}
SHORT = dict(FORCE_WALK, SCHWZ_SWEEP_T="512", SCHWZ_SWEEP_L="4")
SHAPES = {
    # name: (grid, slabs (1: the whole grid; 3: the middle slab's local matrix), switches at upload, generic mode)
    "walk_small": ((256, 4, 12), 1, SHORT, False),
    "gen_200x9": ((200, 9, 11), 1, FORCE_WALK, True),
    "slab_middle": ((256, 4, 36), 3, SHORT, False),
}
_REFS = {}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _matrix(schwz, oracle, shape, slabs):
    if slabs == 1:
        return oracle.laplacian3d(*shape)
    prob = schwz.Problem.laplacian(3, *shape)
    sd = schwz.Subdomain(prob, slabs, slabs // 2, 2, schwz.partition_regular(shape[0] * shape[1] * shape[2], slabs))
    return sd.local_matrix()


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
def test_walk_entry_against_the_chunk_launches(schwz, oracle, torch_cuda, monkeypatch, name):
    hp.require_extended_precision()
    torch = torch_cuda
    shape, slabs, env, gen = SHAPES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SCHWZ_CG_DEFERX", "2")
    rp, col, val = _matrix(schwz, oracle, shape, slabs)
    n = len(rp) - 1
    A = schwz.Csr(rp, col, val)
    assert A.format() == 3 and A.symmetric() and A.sweep_slots() > 0 and A.sweep_left_out() == 0
    assert ((shape[0] * shape[1]) % 512 != 0) == gen
    cg = schwz.Pcg(A, 1)
    rng = np.random.default_rng(18)
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)

    def solve(sweep, iters, start, rtol=0.0, rhs=b, first=x0):
        monkeypatch.setenv("SCHWZ_CG_SWEEP", sweep)
        monkeypatch.setenv("SCHWZ_CG_SWEEPSTART", start)
        d_b, d_x = _dev(torch, rhs), _dev(torch, first)
        it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), rtol, iters)
        return it, rn, d_x.cpu().numpy(), cg.flavour()

    # one iteration, chunk-by-chunk start: the same bits
    it0, rn0, x_ref, fl0 = solve("0", 1, "0")
    it1, rn1, x_sw, fl1 = solve("1", 1, "0")
    print("%s: 1 iteration, flavours %d / %d, residual norms %.17g / %.17g" % (name, fl0, fl1, rn0, rn1))
    assert fl0 & 24 == 0 and fl1 & 56 == 24, (fl0, fl1)
    assert it0 == it1 == 1
    assert np.array_equal(x_ref, x_sw)
    # 2, 7 and 20 iterations, both starts, inside the extended-precision bound
    ref = _references(name, rp, col, val, b, x0)
    for iters in ITERS:
        x_ld, x_64 = ref[LD][0][iters], ref[np.float64][0][iters]
        scale = float(np.abs(x_ld).max())
        dev = max(float(np.abs(x_64 - x_ld).max()) / scale, iters * 2.0 ** -52)
        it0, _, x_ref, _ = solve("0", iters, "0")
        assert float(np.abs(x_ref - x_ld).max()) / scale <= MARGIN * dev
        for start in ("0", "1"):
            it1, _, x_sw, fl = solve("1", iters, start)
            assert fl & 56 == (56 if start == "1" else 24), (start, fl)
            err_ld = float(np.abs(x_sw - x_ld).max()) / scale
            err = float(np.abs(x_sw - x_ref).max()) / scale
            print("%s: %d iterations, start %s, flavour %d: walk - chunks %.2e, walk - extended %.2e, dev %.2e"
                  % (name, iters, start, fl, err, err_ld, dev))
            assert it0 == it1 == iters
            assert err_ld <= MARGIN * dev and err <= 2.0 * MARGIN * dev, (iters, start, err, err_ld, dev)
    # a start residual of exactly zero: no iteration, x untouched
    xi = rng.integers(-8, 9, n).astype(np.float64)
    bi = np.zeros(n)
    np.add.at(bi, np.repeat(np.arange(n), np.diff(rp)), val * xi[col])   # small integers: exact in any order
    for sweep, start in (("0", "0"), ("1", "0"), ("1", "1")):
        it, rn, x_out, fl = solve(sweep, 5, start, rhs=bi, first=xi)
        print("%s: zero start residual, sweep %s start %s: %d iterations, norm %g, flavour %d" % (name, sweep, start, it, rn, fl))
        assert it == 0 and rn == 0.0
        assert np.array_equal(x_out, xi)
    # a stop on a tolerance: the iteration count
    it0, _, x_ref, _ = solve("0", n, "0", 1e-9)
    for start in ("0", "1"):
        it1, _, x_sw, _ = solve("1", n, start, 1e-9)
        print("%s: rtol 1e-9, start %s: %d / %d iterations" % (name, start, it0, it1))
        assert 1 < it0 < n and abs(it0 - it1) <= 1


def test_walk_entry_in_a_three_slab_run(schwz, oracle, torch_cuda, monkeypatch):
    """256 x 4 x 36 in three z slabs, overlap 2, eight CG iterations per local solve, five outer iterations, in one
    process: the middle slab's solves start with the fused check residual, i.e. the DUAL form of the start walk plus
    the listed launch of the flagged planes.  Walk against SCHWZ_CG_SWEEP=0: the same iteration count; solution and
    residual history to 1e-8 of the CPU oracle each (the bound of smoke()), hence to 2e-8 of each other."""
    torch = torch_cuda
    shape, P = (256, 4, 36), 3
    for k, v in dict(SHORT, SCHWZ_CG_DEFERX="2").items():
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
