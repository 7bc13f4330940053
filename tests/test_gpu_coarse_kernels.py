"""The kernels of the coarse correction (csrc/coarse.hip, schwz_ras_coarse_apply), launch by launch, at their edges.

  GEMV      schwz_coarse_solve against the longdouble product row by row, at hp.coarse_gemv_bound: nc = 1 .. 4096, odd
            (coarse_gemv_kernel<false>) and even (16-byte pairs), around the 64 lanes of a wave and the 128 of a pair pass.
  residual  schwz_ras_coarse_residual against the DEFINITION s_a = sum_{i in a} (b_i - sum_j A_ij x~_j) in longdouble
            (hp.coarse_residual: no W is restated), at hp.coarse_residual_bound: aggregates of 0, 1, 2 and 3 pieces,
            pieces of 2048 entries and of one, scattered aggregates with overlap slots in W, empty subdomains.
  apply     schwz_ras_coarse_apply bit for bit (one rounded addition per entry: hp.coarse_apply): odd and even nx and
            ny, ny < nx and ny == nx, nc = 4096 and 1, the stride loop past the grid cap, every home of y.
  bytes     schwz_ras_algorithmic_bytes(sd, 2) from the counts of the host restatement.

Both bounds hold for any summation order and nothing in them is measured on a kernel; every case asserts its shape
conditions -- piece counts, parities, sizes -- on the host before the first launch, and prints its largest
error / bound."""
import numpy as np
import pytest

import cg_child as cc
import hp_reference as hp
from test_gpu_ras_steps import StepRig, bits, global_case

pytestmark = pytest.mark.gpu

SCATTERED = {"band_p3": (5, 4, 6), "nonsym_band_p3": (5, 4, 6), "scaled_band_p3": (5, 4, 6), "ani4_graph_p3": (5, 4, 6),
             "arrow_p2": (3, 4)}      # aggregates per subdomain
GRID_CAP_SLOTS = 2097152              # kMaxGrid / 2 workgroups x 256 lanes x 4 pairs x 2 slots


# ---- rigs ----------------------------------------------------------------------------------------------------------

class Rig(StepRig):
    """StepRig's get / put over a matrix given here: every subdomain of the partition on the device, the rhs +-u."""

    def __init__(self, schwz, torch, matrix, P=1, fr=None, env=None, seed=0, **device_kw):
        self.schwz, self.torch, self.P = schwz, torch, P
        prob = matrix if isinstance(matrix, schwz.Problem) else schwz.Problem.from_csr(*matrix)
        self.prob, self.N = prob, prob.N
        fr = schwz.partition_regular(prob.N, P) if fr is None else fr
        self.which = list(range(P))
        self.sds = {me: schwz.Subdomain(prob, P, me, 2, fr) for me in self.which}
        self.rhs_global = hp.pow2_operands(np.random.default_rng(3000 + seed), self.N)
        self.rhs, self.x, self.idx, self.l2g = {}, {}, {}, {}
        kw = dict(precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=3)
        kw.update(device_kw)
        with cc.upload_env(env or {}):
            for me, sd in self.sds.items():
                self.l2g[me] = sd.local_to_global
                self.rhs[me] = self.rhs_global[self.l2g[me][:sd.local_size_x]].copy()
                sd.to_device(self.rhs[me], **kw)
                self.idx[me] = torch.arange(max(sd.local_size_x + sd.halo_size, 1), dtype=torch.int32, device="cuda")


class CoarseVec:
    """s (0) and c (1) of a schwz.Coarse through its pointers."""

    def __init__(self, schwz, torch, coarse):
        self.schwz, self.torch, self.coarse = schwz, torch, coarse
        self.idx = torch.arange(coarse.nc, dtype=torch.int32, device="cuda")

    def get(self, which):
        p, cnt = self.coarse.vector(which)
        assert cnt == self.coarse.nc
        t = self.torch.empty(cnt, dtype=self.torch.float64, device="cuda")
        self.schwz.gather(cnt, self.idx.data_ptr(), p, t.data_ptr())
        self.torch.cuda.synchronize()
        return t.cpu().numpy()

    def put(self, which, a):
        p, cnt = self.coarse.vector(which)
        assert len(a) == cnt == self.coarse.nc
        t = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        self.schwz.gather(cnt, self.idx.data_ptr(), t.data_ptr(), p)
        self.torch.cuda.synchronize()


def get(rig, me, which):
    return rig.get(me, which) if rig.sds[me].vector(which)[1] else np.zeros(0)


def put(rig, me, which, a):
    if len(a):
        rig.put(me, which, a)


def slots(sd):
    return sd.local_size_x + sd.halo_size


def set_aggregates(rig, interior_ids, first):
    """interior_ids[me]: the global aggregate id of every interior row of subdomain me, inside [first[me],
    first[me + 1]).  Every slot takes the id its owner gave it.  Returns slot ids per subdomain and nc."""
    agg_global = np.full(rig.N, -1, dtype=np.int64)
    for me, sd in rig.sds.items():
        agg_global[rig.l2g[me][:sd.local_size]] = interior_ids[me]
    assert (agg_global >= 0).all()
    nc, slot_agg = int(first[-1]), {}
    for me, sd in rig.sds.items():
        slot_agg[me] = agg_global[rig.l2g[me]]
        sd.coarse_set_aggregates(slot_agg[me], int(first[me]), int(first[me + 1] - first[me]), nc)
    return slot_agg, nc


def reference(rig, me, x, agg_local, m):
    """(s, e, W restated) of subdomain me for the slot values x, from its local matrix and rhs."""
    sd = rig.sds[me]
    n = sd.local_size
    rp, col, val = sd.local_matrix()
    rp = rp[:n + 1]
    col, val = col[:rp[n]], val[:rp[n]]
    assert n == 0 or col.max() < sd.local_size_x
    b = rig.rhs[me][:n]
    s = hp.coarse_residual(rp, col, val, x, b, agg_local, m)
    e = hp.coarse_residual_bound(rp, col, val, x, b, agg_local, m)
    return s, e, hp.coarse_w(rp, col, val, b, agg_local, m)


def check_segment(got, s, e, what):
    if len(s) == 0:
        return 0.0
    assert np.isfinite(got).all(), what
    assert (e > 0).all()                                        # (every aggregate has a row with a nonzero rhs)
    q = np.abs(got.astype(hp.LD) - s) / e
    a = int(np.argmax(q))
    assert q[a] <= 1.0, ("%s: aggregate %d is %.3g times its bound off: got %r, reference %r"
                         % (what, a, float(q[a]), got[a], s[a]))
    return float(q[a])


def expected_bytes(sd, nw, m, nc, own_y):
    return 20 * nw + 16 * m + 8 * m * nc + 16 * nc + 18 * slots(sd) + (16 * sd.local_size_x if own_y else 0)


# ---- GEMV ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", [1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 255, 4095, 4096])
def test_gemv_row_by_row(schwz, torch_cuda, nc):
    """M_ij = +-u 2^(e_i + f_j), s_j = +-u 2^-f_j, e and f in [-20, 20]: badly scaled operands, comparable terms in
    every row.  M is no inverse of anything: the kernel is a matrix-vector product."""
    hp.require_extended_precision()
    rng = np.random.default_rng(900 + nc)
    e, f = rng.integers(-20, 21, nc), rng.integers(-20, 21, nc)
    M = hp.pow2_operands(rng, nc * nc, exps=(e[:, None] + f[None, :]).reshape(-1)).reshape(nc, nc)
    s = hp.pow2_operands(rng, nc, exps=-f)
    ref, mag = hp.coarse_gemv(M, s)
    bound = hp.coarse_gemv_bound(mag, nc)
    assert (mag > 0).all() and (bound > 0).all()
    coarse = schwz.Coarse(M)
    v = CoarseVec(schwz, torch_cuda, coarse)
    v.put(0, s)
    v.put(1, np.full(nc, np.nan))
    coarse.solve()
    c = v.get(1)
    assert np.isfinite(c).all()
    q = np.abs(c.astype(hp.LD) - ref) / bound
    i = int(np.argmax(q))
    assert q[i] <= 1.0, "nc %d: row %d is %.3g times its bound off: got %r, reference %r" % (nc, i, float(q[i]), c[i], ref[i])
    assert np.array_equal(bits(v.get(0)), bits(s)), "s changed"
    v.put(1, np.full(nc, np.nan))
    coarse.solve()
    assert np.array_equal(bits(v.get(1)), bits(c)), "a second call gives other bits"
    print("\ngemv nc %4d (%s kernel): max error / bound %.3g (row %d)" % (nc, "pairs" if nc % 2 == 0 else "odd", float(q[i]), i))


# ---- coarse residual ---------------------------------------------------------------------------------------------------

def run_residual(schwz, torch, rig, interior_local, counts, x, tag):
    """interior_local[me]: local aggregate ids of the interior rows; counts[me] = m.  x[me]: the slot values.  Sets
    the aggregates, runs the residual of every subdomain twice into a NaN-filled s and checks every segment.
    Returns (coarse, CoarseVec, slot ids, first, restated W per subdomain, worst ratio)."""
    hp.require_extended_precision()
    first = np.concatenate([[0], np.cumsum([counts[me] for me in sorted(rig.sds)])]).astype(np.int64)
    slot_agg, nc = set_aggregates(rig, {me: first[me] + interior_local[me] for me in rig.sds}, first)
    refs = {me: reference(rig, me, x[me][:rig.sds[me].local_size_x], interior_local[me], counts[me]) for me in rig.sds}
    coarse = schwz.Coarse(np.zeros((nc, nc)))
    v = CoarseVec(schwz, torch, coarse)
    for me in rig.sds:
        put(rig, me, 0, x[me])
    runs = []
    for _ in range(2):
        v.put(0, np.full(nc, np.nan))
        for me, sd in rig.sds.items():
            sd.coarse_residual(coarse)
        runs.append(v.get(0))
    s = runs[0]
    assert np.isfinite(s).all(), (tag, "an entry of s was not written")
    assert np.array_equal(bits(runs[1]), bits(s)), (tag, "a second call gives other bits")
    worst = 0.0
    for me in rig.sds:
        worst = max(worst, check_segment(s[first[me]:first[me + 1]], refs[me][0], refs[me][1], "%s subdomain %d" % (tag, me)))
        assert np.array_equal(bits(get(rig, me, 0)), bits(x[me])), (tag, me, "x~ changed")
    return coarse, v, slot_agg, first, {me: refs[me][2] for me in rig.sds}, worst


_pieces = {}


def pieces_rig(schwz, torch):
    """hp.sym_band_matrix(16384, 6, 40), one subdomain; kept for the tests that plan it again."""
    if "rig" not in _pieces:
        rng = np.random.default_rng(7)
        _pieces["rig"] = Rig(schwz, torch, hp.sym_band_matrix(16384, 6, 40, rng), seed=7)
        _pieces["x"] = hp.pow2_operands(rng, 16384)
    return _pieces["rig"], _pieces["x"]


def test_residual_of_aggregates_of_one_two_and_three_pieces(schwz, torch_cuda):
    rig, x = pieces_rig(schwz, torch_cuda)
    sd = rig.sds[0]
    assert sd.local_size == sd.local_size_x == slots(sd) == 16384
    rp, col, val = sd.local_matrix()
    targets = (int(rp[1]), 2047, 2048, 2049, 4096, 4097)
    agg = hp.aggregates_by_w_count(rp, col, targets)
    m = len(targets) + 1
    assert m == 7 and m % 2 == 1 and set(agg) == set(range(m))
    w_ptr, w_slot, w_val, beta = hp.coarse_w(rp, col, val, rig.rhs[0], agg, m)
    nw = np.diff(w_ptr)
    assert tuple(nw[:6]) == targets, nw
    pieces, piece_ptr = hp.coarse_pieces(w_ptr)
    sizes = [b1 - b0 for _, b0, b1 in pieces]
    assert {1, 2, 3} <= set(np.diff(piece_ptr)) and 2048 in sizes and 1 in sizes
    assert sd.algorithmic_bytes(2) == 0                       # no aggregates yet
    own_y = sd.y_form() != 1
    coarse, v, slot_agg, first, w, worst = run_residual(schwz, torch_cuda, rig, {0: agg}, {0: m}, {0: x}, "pieces")
    assert sd.algorithmic_bytes(2) == expected_bytes(sd, int(w_ptr[-1]), m, m, own_y)
    print("\nresidual pieces: W entries per aggregate %s, pieces per aggregate %s, piece sizes %s: max error / bound %.3g"
          % (nw.tolist(), np.diff(piece_ptr).tolist(), sorted(set(sizes)), worst))


def scattered_setup(schwz, torch, name):
    rig = StepRig(schwz, torch, name, {}, connect=False)
    counts = dict(enumerate(SCATTERED[name]))
    rng = np.random.default_rng(sum(name.encode()) + 6000)
    interior = {}
    for me, sd in rig.sds.items():
        ids = rng.integers(0, counts[me], sd.local_size)
        ids[:counts[me]] = np.arange(counts[me])              # no aggregate without a row
        interior[me] = ids
    return rig, counts, interior, rng


@pytest.mark.parametrize("name", sorted(SCATTERED))
def test_residual_of_scattered_aggregates(schwz, torch_cuda, name):
    """Every interior row assigned at random to one of its subdomain's aggregates: the gathered slots are not
    contiguous, and slots of the overlap stand in W."""
    rig, counts, interior, rng = scattered_setup(schwz, torch_cuda, name)
    x = {me: hp.pow2_operands(rng, slots(sd)) for me, sd in rig.sds.items()}
    assert len(rig.sds) == len(SCATTERED[name])
    coarse, v, slot_agg, first, w, worst = run_residual(schwz, torch_cuda, rig, interior, counts, x, name)
    longest = 0
    for me, sd in rig.sds.items():
        w_ptr, w_slot = w[me][0], w[me][1]
        assert sd.overlap_size > 0 and (w_slot >= sd.local_size).any(), (name, me, "no overlap slot in W")
        assert (np.diff(w_slot) != 1).any()                    # not a contiguous range of slots
        longest = max(longest, int(np.diff(w_ptr).max()))
        assert sd.algorithmic_bytes(2) == expected_bytes(sd, int(w_ptr[-1]), counts[me], int(first[-1]), True)
    if name == "arrow_p2":
        assert longest > 1400                                   # the long row in one aggregate
    print("\nresidual scattered %-16s nc %2d, longest aggregate %d W entries: max error / bound %.3g"
          % (name, int(first[-1]), longest, worst))


def block_matrix(every_third):
    """256 diagonal blocks [[1, -1], [-1, 1]] (every column sum an exact zero); every_third: the blocks of every third
    aggregate of four rows are [[2, -1], [-1, 2]]."""
    n = 512
    agg = np.arange(n) // 4
    d = np.where(every_third & (agg % 3 == 1), 2.0, 1.0)
    rp = np.arange(0, 2 * n + 1, 2, dtype=np.int32)
    col = (np.arange(n)[:, None] // 2 * 2 + np.arange(2)[None, :]).astype(np.int32).reshape(-1)
    val = np.where(col == np.repeat(np.arange(n), 2), np.repeat(d, 2), -1.0)
    return (rp, col, val), agg


@pytest.mark.parametrize("every_third", [False, True])
def test_residual_of_aggregates_without_a_piece(schwz, torch_cuda, every_third):
    """W_aj = 1 - 1 is an exact zero and is dropped: piece_ptr[a] == piece_ptr[a + 1], and with no piece at all no
    partial launch.  s_a is then beta_a, the rhs summed over the rows in ascending order, bit for bit.  The matrix is
    singular: the local solver is CG without a preconditioner, and nothing here solves with it."""
    matrix, agg = block_matrix(every_third)
    rig = Rig(schwz, torch_cuda, matrix, precond=schwz.capi.PRECOND_NONE, seed=11 + every_third)
    sd = rig.sds[0]
    rp, col, val = sd.local_matrix()
    w_ptr, w_slot, w_val, beta = hp.coarse_w(rp, col, val, rig.rhs[0], agg, 128)
    pieces, piece_ptr = hp.coarse_pieces(w_ptr)
    empty = np.diff(piece_ptr) == 0
    if every_third:
        assert empty[0] and not empty[1] and empty[2] and empty.sum() == 85 and len(pieces) == 43 and w_ptr[-1] == 172
    else:
        assert empty.all() and len(pieces) == 0 and w_ptr[-1] == 0
    b = rig.rhs[0]
    assert np.array_equal(beta, ((b[0::4] + b[1::4]) + b[2::4]) + b[3::4])
    x = hp.pow2_operands(np.random.default_rng(12), 512, -20, 20)
    own_y = sd.y_form() != 1
    coarse, v, slot_agg, first, w, worst = run_residual(schwz, torch_cuda, rig, {0: agg}, {0: 128}, {0: x}, "no pieces")
    s = v.get(0)
    assert np.array_equal(bits(s[empty]), bits(beta[empty])), "an aggregate without a piece is not its beta"
    assert every_third == bool((s != beta).any())
    assert sd.algorithmic_bytes(2) == expected_bytes(sd, int(w_ptr[-1]), 128, 128, own_y)    # (the device's W count)
    print("\nresidual no pieces (every third aggregate with entries: %s): %d of 128 aggregates without a piece, %d pieces: "
          "max error / bound %.3g" % (every_third, int(empty.sum()), len(pieces), worst))


def test_residual_and_apply_with_empty_subdomains(schwz, torch_cuda):
    """Three rows on five subdomains: the calls on a subdomain without a row or an aggregate succeed and do nothing."""
    rp, col = np.array([0, 2, 5, 7], dtype=np.int32), np.array([0, 1, 0, 1, 2, 1, 2], dtype=np.int32)
    val = np.array([2.0, -1.0, -1.0, 2.0, -1.0, -1.0, 2.0])
    rig = Rig(schwz, torch_cuda, (rp, col, val), P=5)
    sizes = [sd.local_size for _, sd in sorted(rig.sds.items())]
    assert sum(sizes) == 3 and sizes.count(0) >= 2, sizes
    counts = {me: rig.sds[me].local_size for me in rig.sds}
    interior = {me: np.arange(counts[me]) for me in rig.sds}
    rng = np.random.default_rng(13)
    x = {me: hp.pow2_operands(rng, slots(sd)) for me, sd in rig.sds.items()}
    coarse, v, slot_agg, first, w, worst = run_residual(schwz, torch_cuda, rig, interior, counts, x, "empty subdomains")
    c = hp.pow2_operands(rng, 3, -20, 20)
    v.put(1, c)
    for me, sd in rig.sds.items():
        y = hp.pow2_operands(rng, sd.local_size_x, -20, 20)
        put(rig, me, 2, y)
        sd.coarse_apply(coarse)                                 # (SCHWZ_OK on the empty ones: check() raises otherwise)
        want_x, want_y = hp.coarse_apply(x[me], y, c, slot_agg[me])
        got_x, got_y = get(rig, me, 0), get(rig, me, 2)
        assert np.isfinite(got_x).all() and np.isfinite(got_y).all()
        assert np.array_equal(bits(got_x), bits(want_x)) and np.array_equal(bits(got_y), bits(want_y)), me
    print("\nresidual empty subdomains: interior rows %s: max error / bound %.3g" % (sizes, worst))


# ---- apply -------------------------------------------------------------------------------------------------------------

def check_apply(rig, me, v, slot_agg, rng, tag, y_is_x=False):
    """x~, y and c written through their pointers with exponents spread over [-20, 20]; one apply; bit for bit."""
    sd = rig.sds[me]
    nc = v.coarse.nc
    c = hp.pow2_operands(rng, nc, -20, 20)
    x = hp.pow2_operands(rng, slots(sd), -20, 20)
    y = x[:sd.local_size_x] if y_is_x else hp.pow2_operands(rng, sd.local_size_x, -20, 20)
    assert (sd.vector(0)[0] == sd.vector(2)[0]) == y_is_x, tag
    v.put(1, c)
    s_before = v.get(0)
    put(rig, me, 0, x)
    if not y_is_x:
        put(rig, me, 2, y)
    sd.coarse_apply(v.coarse)
    want_x, want_y = hp.coarse_apply(x, y, c, slot_agg)
    assert (want_x != x).all() and (want_y != y).all()         # no c absorbed: a skipped slot shows
    got_x, got_y = get(rig, me, 0), get(rig, me, 2)
    bad = np.nonzero(bits(got_x) != bits(want_x))[0]
    assert len(bad) == 0, "%s: x~ differs in %d of %d slots, first %d: got %r, want %r (x~ %r, c %r)" % (
        tag, len(bad), len(x), bad[0], got_x[bad[0]], want_x[bad[0]], x[bad[0]], c[slot_agg[bad[0]]])
    bad = np.nonzero(bits(got_y) != bits(want_y))[0]
    assert len(bad) == 0, "%s: y differs in %d of %d entries, first %d: got %r, want %r (y %r, c %r)" % (
        tag, len(bad), len(y), bad[0], got_y[bad[0]], want_y[bad[0]], y[bad[0]], c[slot_agg[bad[0]]])
    assert np.array_equal(bits(v.get(1)), bits(c)) and np.array_equal(bits(v.get(0)), bits(s_before)), (tag, "c or s changed")


def test_the_scattered_cases_hold_every_parity_of_nx_and_ny(schwz):
    """On the host alone: together the subdomains of the apply cases with ny = local_size_x < nx have an even and an
    odd nx, each with an even and an odd ny (the pair branch that stops inside x~, and its single-entry branch); no
    partition with an explicit first_row is needed for that."""
    seen = set()
    for name in sorted(SCATTERED):
        rp, col, val, P, fr, _ = global_case(name)
        prob = schwz.Problem.from_csr(rp, col, val)
        if isinstance(fr, str):
            prob, _, fr = prob.permute(prob.partition_graph(P), P)
        elif fr is None:
            fr = schwz.partition_regular(prob.N, P)
        for me in range(P):
            sd = schwz.Subdomain(prob, P, me, 2, fr)
            if sd.local_size_x < slots(sd):
                seen.add((slots(sd) % 2, sd.local_size_x % 2))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen


@pytest.mark.parametrize("name", sorted(SCATTERED))
def test_apply_on_general_matrices(schwz, torch_cuda, name):
    rig, counts, interior, rng = scattered_setup(schwz, torch_cuda, name)
    first = np.concatenate([[0], np.cumsum([counts[me] for me in sorted(rig.sds)])]).astype(np.int64)
    slot_agg, nc = set_aggregates(rig, {me: first[me] + interior[me] for me in rig.sds}, first)
    v = CoarseVec(schwz, torch_cuda, schwz.Coarse(np.zeros((nc, nc))))
    shapes = []
    for me, sd in rig.sds.items():
        assert sd.y_form() == 0
        shapes.append((slots(sd), sd.local_size_x))
        check_apply(rig, me, v, slot_agg[me], rng, "%s subdomain %d" % (name, me))
    print("\napply %-16s nc %2d, (nx, ny) per subdomain %s: bit for bit" % (name, nc, shapes))


def test_large_nc_and_planning_again(schwz, torch_cuda):
    """The pieces matrix planned again: four consecutive rows per aggregate (nc = 4096: 32 KiB of c staged in 16 trips,
    ids 0 and 4095), then one aggregate (nc = 1, eight pieces).  schwz_ras_coarse_set_aggregates replaces the plan."""
    rig, x = pieces_rig(schwz, torch_cuda)
    sd = rig.sds[0]
    rng = np.random.default_rng(21)
    for nc, agg in ((4096, np.arange(16384) // 4), (1, np.zeros(16384, dtype=np.int64))):
        assert agg.min() == 0 and agg.max() == nc - 1 == (4095 if nc > 1 else 0)
        coarse, v, slot_agg, first, w, worst = run_residual(schwz, torch_cuda, rig, {0: agg}, {0: nc}, {0: x}, "nc %d" % nc)
        pieces, piece_ptr = hp.coarse_pieces(w[0][0])
        assert len(pieces) == (4096 if nc > 1 else 8)
        assert sd.algorithmic_bytes(2) == expected_bytes(sd, int(w[0][0][-1]), nc, nc, sd.y_form() != 1)
        check_apply(rig, 0, v, slot_agg[0], rng, "nc %d" % nc)
        print("\nplanned again with nc %4d: %d pieces, residual max error / bound %.3g, apply bit for bit"
              % (nc, len(pieces), worst))


def test_apply_and_residual_past_the_grid_cap(schwz, torch_cuda):
    """2-D Laplacian 1449 x 1449: 2 099 601 slots, odd, more than the 2 097 152 that 1024 workgroups cover at four pairs
    a lane: the stride loop makes a second trip.  SCHWZ_CG_DEFERX=0 at the upload: y is a buffer of its own, ny == nx."""
    hp.require_extended_precision()
    n1 = 1449
    rig = Rig(schwz, torch_cuda, schwz.Problem.laplacian(2, n1, n1), env={"SCHWZ_CG_DEFERX": "0"}, seed=31)
    sd = rig.sds[0]
    N = n1 * n1
    assert slots(sd) == sd.local_size_x == N == 2099601 and N % 2 == 1 and N > GRID_CAP_SLOTS
    assert sd.y_form() == 0
    agg = np.arange(N) * 100 // N
    assert agg.max() == 99 and len(np.unique(agg)) == 100
    rng = np.random.default_rng(32)
    x = hp.pow2_operands(rng, N)
    with cc.upload_env({"SCHWZ_CG_DEFERX": "0"}):
        slot_agg, nc = set_aggregates(rig, {0: agg}, np.array([0, 100]))
        v = CoarseVec(schwz, torch_cuda, schwz.Coarse(np.zeros((100, 100))))
        rp, col, val = sd.local_matrix()
        s_ref = hp.coarse_residual(rp, col, val, x, rig.rhs[0], agg, 100)
        e = hp.coarse_residual_bound(rp, col, val, x, rig.rhs[0], agg, 100)
        put(rig, 0, 0, x)
        v.put(0, np.full(100, np.nan))
        sd.coarse_residual(v.coarse)
        worst = check_segment(v.get(0), s_ref, e, "past the grid cap")
        assert sd.y_form() == 0
        check_apply(rig, 0, v, slot_agg[0], rng, "past the grid cap")
    print("\napply past the grid cap: %d slots, ny == nx odd: bit for bit; residual max error / bound %.3g" % (N, worst))


HOMES = ("cholesky", "lu", "gmres", "bicgstab", "cg_f32", "chebyshev", "cg_deferx0", "cg_state_a", "cg_state_b")


def home_rig(schwz, torch, home, P):
    capi = schwz.capi
    kw = {}
    if home == "cholesky":
        kw = dict(local_solver=capi.SOLVER_DIRECT)
    elif home == "lu":
        kw = dict(local_solver=capi.SOLVER_DIRECT_LU)
    elif home in ("gmres", "bicgstab"):
        kw = dict(non_symmetric=True, restart_iter=3)
    rig = Rig(schwz, torch, schwz.Problem.laplacian(3, 12, 12, 12), P=P, seed=41, **kw)
    for sd in rig.sds.values():
        if home == "bicgstab":
            sd.set_nonsym_solver(capi.NONSYM_BICGSTAB)
        elif home == "cg_f32":
            sd.set_local_precision(capi.PRECISION_F32)
        elif home == "chebyshev":
            sd.set_sym_solver(capi.SYM_CHEBYSHEV)
    return rig


def run_home(schwz, torch, home, P, monkeypatch):
    monkeypatch.setenv("SCHWZ_CG_DEFERX", "0" if home == "cg_deferx0" else ("2" if home.startswith("cg_state") else "1"))
    rig = home_rig(schwz, torch, home, P)
    N = 1728
    agg = np.arange(N) // 64                                    # 27 aggregates (odd), 9 per slab of 576 rows
    first = np.arange(P + 1) * (27 // P)
    interior = {me: agg[rig.l2g[me][:sd.local_size]] for me, sd in rig.sds.items()}
    for me in rig.sds:
        assert interior[me].min() == first[me] and interior[me].max() == first[me + 1] - 1
    for sd in rig.sds.values():
        assert sd.algorithmic_bytes(2) == 0
    slot_agg, nc = set_aggregates(rig, interior, first)
    v = CoarseVec(schwz, torch, schwz.Coarse(np.zeros((27, 27))))
    rng = np.random.default_rng(42)
    want_form = {"cg_state_a": 1, "cg_state_b": 2}.get(home, 0) if P == 1 else 0
    nws = {me: int(reference(rig, me, np.zeros(sd.local_size_x), interior[me] - first[me], 27 // P)[2][0][-1])
           for me, sd in rig.sds.items()}
    for round_ in range(2):
        for me, sd in rig.sds.items():
            assert (sd.local_size_x < slots(sd)) == (P > 1)
            if round_ == 1:
                # a solve from finite values, then the restriction: y and x~ may have changed buffers
                put(rig, me, 0, hp.pow2_operands(rng, slots(sd)))
                if sd.vector(0)[0] != sd.vector(2)[0]:
                    put(rig, me, 2, hp.pow2_operands(rng, sd.local_size_x))
                sd.local_solve()
                sd.restrict()
            if want_form == 2:
                sd.local_solve()                                # not restricted: y is the other x~ buffer
            torch.cuda.synchronize()
            assert sd.y_form() == want_form, (home, round_, sd.y_form())
            tag = "%s P %d round %d subdomain %d" % (home, P, round_, me)
            check_apply(rig, me, v, slot_agg[me], rng, tag, y_is_x=want_form == 1)
            assert sd.algorithmic_bytes(2) == expected_bytes(sd, nws[me], 27 // P, 27, want_form != 1), tag
    return want_form


@pytest.mark.parametrize("home", HOMES)
def test_apply_in_every_home_of_y(schwz, torch_cuda, monkeypatch, home):
    """lap3d 12 x 12 x 12 on one subdomain, per local solver: apply, check x~ and y; then local_solve, restrict, write
    again, apply, check again.  Where y IS x~ (y_form 1) c is added once; in state B (y_form 2: a solve that was not
    restricted) and with every other solver y is a vector of its own and takes the same launch."""
    form = run_home(schwz, torch_cuda, home, 1, monkeypatch)
    print("\napply home %-10s y_form %d, nx == ny == 1728, nc 27: bit for bit before and after a solve" % (home, form))


@pytest.mark.parametrize("home", ["cg_deferx0", "gmres"])
def test_apply_on_three_subdomains_with_halo(schwz, torch_cuda, monkeypatch, home):
    run_home(schwz, torch_cuda, home, 3, monkeypatch)
    print("\napply home %-10s three subdomains, ny < nx: bit for bit before and after a solve" % home)
