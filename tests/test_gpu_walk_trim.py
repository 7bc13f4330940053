"""The z-sweep walks on segment tables with uneven cuts (SCHWZ_SWEEP_TRIM, walk_segment_table in csrc/coding_plan.cpp):
the kernels read {band, p0, p1, rows} per workgroup and take pieces of any length, so a table whose late pieces are
shorter must give what the equal pieces give -- up to the order in which the partial sums of alpha, beta and the norms
are folded, since trimming regroups the rows behind each workgroup's partial sum.

Shapes, as small as the trimmed path allows.  A run is only cut unevenly when its equal pieces have 16 positions or
more and the table has more segments than CUs, so: 40 planes, SCHWZ_SWEEP_L = SCHWZ_SWEEP_LDIR = 20 (two pieces of 20
per band), tables planned for three CUs (SCHWZ_SWEEP_CUS=3: the last piece's workgroups are the late round), and 200 per
mille, which moves the cut from position 21 to 23 (pieces of 22 and 18; tests/drivers/walk_trim_driver.cpp holds the
same geometry to its invariants on the CPU, cases gpu_256x4x40 and gpu_200x9x40).
  256 x 4 x 40   planes of two whole chunks, bands of 512 rows
  200 x 9 x 40   planes that are not whole chunks: byte pattern ids, a partial last band, the generic walk
  256 x 4 x 96 in three slabs, overlap 2: the middle slab has both neighbours (chained overlap planes, fused check
                 residual at the start); runs of 33 to 36 positions, two pieces of 17 or 18 per band

Bounds: those of tests/test_gpu_walk_prologue.py, whose helpers and MARGIN are used here -- one iteration from a
chunk-by-chunk start is bit for bit; later, walk and chunk launches each lie within MARGIN x dev of the
extended-precision iterate and hence within twice that of each other.  The same systems are then solved with
SCHWZ_SWEEP_TRIM=0 in the same process: the same bounds, and the same slot counts."""
import numpy as np
import pytest

import hp_reference as hp
from test_gpu_walk_prologue import FORCE_WALK, ITERS, LD, MARGIN, _dev, _references

pytestmark = pytest.mark.gpu

TRIM = "200"
SWITCHES = dict(FORCE_WALK, SCHWZ_SWEEP_T="512", SCHWZ_SWEEP_L="20", SCHWZ_SWEEP_LDIR="20", SCHWZ_SWEEP_CUS="3")
SHAPES = {
    # name: (grid, generic mode)
    "trim_256x4x40": ((256, 4, 40), False),
    "trim_200x9x40": ((200, 9, 40), True),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_trimmed_walk_against_the_chunk_launches(schwz, oracle, torch_cuda, monkeypatch, name):
    hp.require_extended_precision()
    torch = torch_cuda
    shape, gen = SHAPES[name]
    for k, v in SWITCHES.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SCHWZ_CG_DEFERX", "2")
    rp, col, val = oracle.laplacian3d(*shape)
    n = len(rp) - 1
    rng = np.random.default_rng(17)
    b = rng.standard_normal(n)
    x0 = 0.1 * rng.standard_normal(n)
    ref = _references(name, rp, col, val, b, x0)
    slots = {}
    for trim in (TRIM, "0"):
        monkeypatch.setenv("SCHWZ_SWEEP_TRIM", trim)   # read at the upload
        A = schwz.Csr(rp, col, val)
        assert A.format() == 3 and A.symmetric() and A.sweep_slots() > 0 and A.sweep_left_out() == 0
        assert ((shape[0] * shape[1]) % 512 != 0) == gen
        slots[trim] = A.sweep_slots()
        cg = schwz.Pcg(A, 1)

        def solve(sweep, iters, start):
            monkeypatch.setenv("SCHWZ_CG_SWEEP", sweep)
            monkeypatch.setenv("SCHWZ_CG_SWEEPSTART", start)
            d_b, d_x = _dev(torch, b), _dev(torch, x0)
            it, rn = cg.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, iters)
            return it, rn, d_x.cpu().numpy(), cg.flavour()

        # one iteration, chunk-by-chunk start: the same products in the same order in every row, alpha_0 from the same sums
        it0, rn0, x_ref, fl0 = solve("0", 1, "0")
        it1, rn1, x_sw, fl1 = solve("1", 1, "0")
        print("%s trim %s: slots %d; 1 iteration, flavours %d / %d, residual norms %.17g / %.17g" % (name, trim, slots[trim], fl0, fl1, rn0, rn1))
        assert fl0 & 24 == 0 and fl1 & 56 == 24, (fl0, fl1)
        assert it0 == it1 == 1
        assert np.array_equal(x_ref, x_sw)
        assert abs(rn0 - rn1) <= n * 2.0 ** -53 * rn0, (rn0, rn1)
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
                print("%s trim %s: %d iterations, start %s: walk - chunks %.2e, walk - extended %.2e, dev %.2e; norms %.17g / %.17g, dev %.2e"
                      % (name, trim, iters, start, err, err_ld, dev, rn0, rn1, dev_r))
                assert it0 == it1 == iters
                assert err_ld <= MARGIN * dev and err <= 2.0 * MARGIN * dev, (trim, iters, start, err, err_ld, dev)
                assert abs(rn1 - r_ld) <= MARGIN * dev_r * r_ld and abs(rn0 - rn1) <= 2.0 * MARGIN * dev_r * r_ld, (trim, iters, start, rn0, rn1, r_ld, dev_r)
    assert slots[TRIM] == slots["0"], slots


def test_trimmed_walk_in_a_three_slab_run(schwz, oracle, torch_cuda, monkeypatch):
    """256 x 4 x 96 in three z slabs, overlap 2, eight CG iterations per local solve, five outer iterations, in one
    process: trimmed walk, equal pieces and SCHWZ_CG_SWEEP=0.  The same iteration count; solution and residual history
    to 1e-8 of the CPU oracle each (the bound of smoke()), hence to 2e-8 of each other; the uploads of every slab's
    local matrix report the same slot counts with and without the trim."""
    torch = torch_cuda
    shape, P = (256, 4, 96), 3
    for k, v in dict(SWITCHES, SCHWZ_CG_DEFERX="2").items():
        monkeypatch.setenv(k, v)

    def run(sweep, trim):
        monkeypatch.setenv("SCHWZ_CG_SWEEP", sweep)
        monkeypatch.setenv("SCHWZ_SWEEP_TRIM", trim)
        s = schwz.Settings(laplacian_dim=3, laplacian_shape=shape)
        m = schwz.Metadata(num_subdomains=P, tolerance=1e-30, max_iters=5, local_precond="block-jacobi",
                           precond_max_block_size=1, local_solver_tolerance=0.0, local_max_iters=8)
        solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
        solver.initialize()
        out = solver.run()
        torch.cuda.synchronize()
        hist = np.asarray(m.post_process_data["global_residual_vector_out"], dtype=np.float64)
        slots = []
        for me in sorted(solver.subdomains):
            A = schwz.Csr(*solver.subdomains[me].local_matrix())
            assert A.format() == 3 and A.sweep_slots() > 0 and A.sweep_left_out() == 0
            slots.append(A.sweep_slots())
        return out, hist, [solver.subdomains[me].cg_flavour() for me in sorted(solver.subdomains)], slots

    out0, h0, fl0, _ = run("0", "0")
    out1, h1, fl1, slots1 = run("1", TRIM)
    out2, h2, fl2, slots2 = run("1", "0")
    print("three slabs: flavours %s / %s / %s, slots %s / %s, final residual %.17g / %.17g / %.17g"
          % (fl0, fl1, fl2, slots1, slots2, out0["residual_norm"], out1["residual_norm"], out2["residual_norm"]))
    assert all(f & 24 == 0 for f in fl0) and all(f & 24 == 24 for f in fl1) and fl1 == fl2, (fl0, fl1, fl2)
    assert out0["iter_count"] == out1["iter_count"] == out2["iter_count"] == 5
    assert slots1 == slots2
    rp, col, val = oracle.laplacian3d(*shape)
    N = len(rp) - 1
    r = oracle.ras_run(rp, col, val, np.ones(N), P, oracle.first_rows_regular(N, P),
                       oracle.make_settings(max_iters=5, tol=1e-30, precond=oracle.PRECOND_JACOBI, local_tol=0.0,
                                            local_max_iters=8))
    scale = np.abs(r["solution"]).max()
    for out in (out0, out1, out2):
        assert np.abs(out["solution"] - r["solution"]).max() <= 1e-8 * scale
    assert h0.shape == h1.shape == h2.shape and h0.size > 0
    for out, h in ((out1, h1), (out2, h2)):
        assert np.abs(out0["solution"] - out["solution"]).max() <= 2e-8 * scale
        assert np.abs(h0 - h).max() <= 2e-8 * np.abs(h0).max()
