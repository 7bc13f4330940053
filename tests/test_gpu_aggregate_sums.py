"""schwz_ras_aggregate_sums (csrc/coarse.hip): s[first_agg + a] = sum of a vector over the rows of aggregate a, the
streaming restriction of the two-level preconditioner inside the outer FGMRES.

The 1-D Laplacian on 15000 rows through SolverRAS.initialize(matrix=...), overlap 2, on one subdomain and on three
in-process subdomains (5000 rows each, so first_agg > 0 occurs), with a coarse_aggregate_vector whose aggregates have
1, 2, 63, 64, 65, 255, 256, 257, cap - 1, cap, cap + 1 and 2 cap + 1 rows (cap = kCoarsePieceCap = 2048: zero to three
pieces' worth, and every count around a wave, a workgroup and a piece) plus one filler per third, and whose rows are
dealt round-robin inside each third: no aggregate is a contiguous run of rows.

Bound, per aggregate of k rows, against the sum in np.longdouble: |s_a - ref_a| <= gamma_(k-1) sum_{i in a} |v_i| with
gamma_k = k u / (1 - k u), u = 2^-53 -- the bound of ANY order of summation (Higham, Accuracy and Stability, eq. 4.4),
so nothing is measured and no margin is added; an aggregate of one row must be exact."""
import numpy as np
import pytest
import scipy.sparse as sp

import stream_rig as rig
from test_gpu_coarse import boxes

pytestmark = pytest.mark.gpu
CAP = 2048
N = 15000
THIRD = N // 3
SIZES = [[2 * CAP + 1, 1, 2, 63], [CAP + 1, CAP, 64, 65, 255], [CAP - 1, 256, 257]]   # per third; a filler takes the rest
U = 2.0 ** -53


def aggregate_vector():
    """One id per global row: inside third t the rows are dealt round-robin to its aggregates while they want rows."""
    ids = np.empty(N, dtype=np.int64)
    base = 0
    for t, sizes in enumerate(SIZES):
        sizes = sizes + [THIRD - sum(sizes)]
        assert sizes[-1] > 0
        left = np.array(sizes)
        out = []
        while left.any():
            live = np.nonzero(left)[0]
            out.append(live)
            left[live] -= 1
        ids[t * THIRD:(t + 1) * THIRD] = base + np.concatenate(out)
        base += len(sizes)
    return ids


_cache = {}


def solver_of(schwz, P):
    if P not in _cache:
        a = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(N, N), format="csr")
        s = schwz.Settings()
        m = schwz.Metadata(num_subdomains=P, tolerance=1e-8, max_iters=5, local_precond="block-jacobi",
                           precond_max_block_size=1, local_solver_tolerance=0.0, local_max_iters=2,
                           coarse_space="aggregates", coarse_aggregate_vector=aggregate_vector())
        solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
        solver.initialize(matrix=(a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float64)),
                          rhs=np.random.default_rng(5).standard_normal(N))
        assert m.permutation is None and s.overlap == 2 and len(solver.subdomains) == P
        _cache[P] = solver
    return _cache[P]


def layout(solver):
    """Per subdomain (global aggregate id of every interior row, first_agg, m), and nc."""
    co = solver._coarse
    out = {}
    for me, sd in sorted(solver.subdomains.items()):
        ids = np.asarray(co["interior"][me], dtype=np.int64)
        first, m = int(co["first"][me]), int(co["first"][me + 1] - co["first"][me])
        assert len(ids) == sd.local_size and ids.min() == first and ids.max() == first + m - 1
        out[me] = (ids, first, m)
    return out, int(co["nc"])


def vectors(ids_global):
    """name -> global vector.  `cancel`: inside every aggregate pairs +t, -t of large t and one or two small entries."""
    rng = np.random.default_rng(77)
    spread = rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-8.0, 8.0, N)
    cancel = np.empty(N)
    for a in np.unique(ids_global):
        rows = np.nonzero(ids_global == a)[0]
        k = len(rows)
        small = 1 if k % 2 else min(2, k)
        t = 1e6 * (1.0 + rng.random((k - small) // 2))
        cancel[rows[:k - small:2]] = t
        cancel[rows[1:k - small:2]] = -t
        cancel[rows[k - small:]] = 1e-3 * (1.0 + rng.random(small))
    return dict(spread=spread, cancel=cancel, ones=np.ones(N))


class Dev:
    """Raw device vectors through the library's own copy launch."""

    def __init__(self, schwz, torch):
        self.schwz, self.torch = schwz, torch

    def read(self, ptr, n):
        out = self.torch.empty(max(n, 1), dtype=self.torch.float64, device="cuda")
        self.torch.cuda.synchronize()
        self.schwz.outer_copy(n, ptr, out.data_ptr())
        self.torch.cuda.synchronize()
        return out.cpu().numpy()[:n]

    def write(self, ptr, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        self.schwz.outer_copy(len(a), t.data_ptr(), ptr)
        self.torch.cuda.synchronize()

    def tensor(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def check_segment(s, ids, first, m, v_local, tag):
    """The bound of the module docstring on the subdomain's m sums; returns the worst error / bound."""
    worst = 0.0
    for a in range(m):
        rows = np.nonzero(ids == first + a)[0]
        k = len(rows)
        vals = v_local[rows].astype(np.longdouble)
        ref = vals.sum(dtype=np.longdouble)
        mag = np.abs(vals).sum(dtype=np.longdouble)
        gamma = np.longdouble((k - 1) * U) / np.longdouble(1.0 - (k - 1) * U)
        err = abs(np.longdouble(s[first + a]) - ref)
        assert err <= gamma * mag, "%s: aggregate %d of %d rows: error %.3e, bound %.3e" % (tag, a, k, float(err), float(gamma * mag))
        if k == 1:
            assert s[first + a] == v_local[rows[0]]
        if mag > 0 and k > 1:
            worst = max(worst, float(err / (gamma * mag)))
    return worst


@pytest.mark.parametrize("P", [1, 3])
def test_sums_meet_the_bound_of_any_order(schwz, torch_cuda, P):
    solver = solver_of(schwz, P)
    dev = Dev(schwz, torch_cuda)
    lay, nc = layout(solver)
    obj = solver._coarse["obj"]
    s_ptr, s_len = obj.vector(0)
    assert s_len == nc == sum(len(x) + 1 for x in SIZES)
    sizes = np.sort(np.concatenate([np.bincount(ids - first, minlength=m) for ids, first, m in lay.values()]))
    wanted = sorted(sum(SIZES, []))
    assert set(wanted) <= set(sizes.tolist()) and {1, 2, 63, 64, 65, 255, 256, 257, CAP - 1, CAP, CAP + 1, 2 * CAP + 1} == set(wanted)
    assert (P == 1) == all(first == 0 for _, first, _ in lay.values())
    for me, (ids, first, m) in lay.items():                       # interleaved: no aggregate is one run of rows
        for a in range(m):
            rows = np.nonzero(ids == first + a)[0]
            assert len(rows) < 2 or rows[-1] - rows[0] > len(rows) - 1
    ids_global = np.empty(N, dtype=np.int64)
    for me, sd in solver.subdomains.items():
        ids_global[sd.local_to_global[:sd.local_size]] = lay[me][0]
    sentinel = -12345.0625
    for name, v in vectors(ids_global).items():
        for me, sd in sorted(solver.subdomains.items()):
            ids, first, m = lay[me]
            v_local = v[np.asarray(sd.local_to_global[:sd.local_size_x], dtype=np.int64)]
            d_v = dev.tensor(v_local)
            dev.write(s_ptr, np.full(nc, sentinel))
            sd.aggregate_sums(obj, d_v.data_ptr())
            s = dev.read(s_ptr, nc)
            tag = "%s, P %d, subdomain %d" % (name, P, me)
            outside = np.ones(nc, dtype=bool)
            outside[first:first + m] = False
            assert (s[outside] == sentinel).all(), tag
            worst = check_segment(s, ids, first, m, v_local, tag)
            print("aggregate_sums %s: worst error / bound %.3e over %d aggregates" % (tag, worst, m))
            if name == "ones":
                assert np.array_equal(s[first:first + m], np.bincount(ids - first, minlength=m).astype(np.float64)), tag
            # twice: the same bits
            dev.write(s_ptr, np.full(nc, sentinel))
            sd.aggregate_sums(obj, d_v.data_ptr())
            assert rig.same(dev.read(s_ptr, nc), s), tag


@pytest.mark.parametrize("P", [1, 3])
def test_any_device_vector_and_beta_untouched(schwz, torch_cuda, P):
    """d_vec may be a buffer of the caller's, the x~ buffer or the vector of id 3: the same bits.  beta of the coarse
    plan -- read through schwz_ras_coarse_residual on a zero x~ -- keeps its bits; the byte model is the tables'."""
    solver = solver_of(schwz, P)
    dev = Dev(schwz, torch_cuda)
    lay, nc = layout(solver)
    obj = solver._coarse["obj"]
    s_ptr, _ = obj.vector(0)
    v = np.random.default_rng(9).standard_normal(N)
    for me, sd in sorted(solver.subdomains.items()):
        ids, first, m = lay[me]
        sd.restart(False)
        dev.write(s_ptr, np.zeros(nc))
        sd.coarse_residual(obj)
        beta = dev.read(s_ptr, nc)[first:first + m]
        assert np.abs(beta).min() > 0
        v_local = v[np.asarray(sd.local_to_global[:sd.local_size_x], dtype=np.int64)]
        d_v = dev.tensor(v_local)
        sd.aggregate_sums(obj, d_v.data_ptr())
        own = dev.read(s_ptr, nc)[first:first + m]
        check_segment(np.concatenate([np.zeros(first), own]), ids, first, m, v_local, "own buffer")
        # the x~ buffer
        px, nx = sd.vector(0)
        assert nx >= sd.local_size_x
        dev.write(px, v_local)
        dev.write(s_ptr, np.zeros(nc))
        sd.aggregate_sums(obj, px)
        assert rig.same(dev.read(s_ptr, nc)[first:first + m], own)
        # the vector of id 3
        b_before = dev.read(sd.vector(3)[0], sd.local_size_x)
        sd.rhs_set(v_local)
        dev.write(s_ptr, np.zeros(nc))
        sd.aggregate_sums(obj, sd.vector(3)[0])
        assert rig.same(dev.read(s_ptr, nc)[first:first + m], own)
        sd.rhs_set(b_before)
        # beta: the same bits as before all of it
        sd.restart(False)
        dev.write(s_ptr, np.zeros(nc))
        sd.coarse_residual(obj)
        assert rig.same(dev.read(s_ptr, nc)[first:first + m], beta)
        pieces = int(sum(-(-c // CAP) for c in np.bincount(ids - first, minlength=m)))
        assert sd.algorithmic_bytes(3) == 12 * sd.local_size + 28 * pieces + 4 * (m + 1) + 8 * m


def test_refusals_and_an_empty_subdomain(schwz, torch_cuda):
    """Another nc and a subdomain without aggregates: SCHWZ_ERR_INVALID; m = 0: SCHWZ_OK, s untouched."""
    dev = Dev(schwz, torch_cuda)
    solver = solver_of(schwz, 1)
    sd = solver.subdomains[0]
    nc = int(solver._coarse["nc"])
    d_v = dev.tensor(np.ones(sd.local_size_x))
    other = schwz.Coarse(np.eye(nc + 1))
    for call in (lambda: sd.aggregate_sums(other, d_v.data_ptr()), lambda: sd.aggregate_sums(solver._coarse["obj"], 0),
                 lambda: sd.aggregate_sums(None, d_v.data_ptr())):
        with pytest.raises(schwz.SchwzError) as e:
            call()
        assert e.value.code == schwz.capi.ERR_INVALID
    # three rows on five subdomains: two of them own nothing
    rp, col = np.array([0, 2, 5, 7], dtype=np.int64), np.array([0, 1, 0, 1, 2, 1, 2], dtype=np.int32)
    prob = schwz.Problem.from_csr(rp, col, np.array([2.0, -1.0, -1.0, 2.0, -1.0, -1.0, 2.0]))
    fr = schwz.partition_regular(3, 5)
    coarse = schwz.Coarse(np.eye(3))
    s_ptr, _ = coarse.vector(0)
    seen_empty = 0
    for me in range(5):
        sub = schwz.Subdomain(prob, 5, me, 2, fr)
        sub.to_device(np.ones(sub.local_size_x), precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=2)
        buf = dev.tensor(np.full(max(sub.local_size_x, 1), 2.5))
        with pytest.raises(schwz.SchwzError) as e:                # no aggregates yet
            sub.aggregate_sums(coarse, buf.data_ptr())
        assert e.value.code == schwz.capi.ERR_INVALID
        own = np.asarray(sub.local_to_global[:sub.local_size], dtype=np.int64)
        slot = np.asarray(sub.local_to_global[:sub.local_size_x + sub.halo_size], dtype=np.int64)
        first = int(own.min()) if len(own) else min(int(fr[me]), 3)
        sub.coarse_set_aggregates(slot, first, len(own), 3)
        dev.write(s_ptr, np.full(3, 7.0))
        sub.aggregate_sums(coarse, buf.data_ptr())
        want = np.full(3, 7.0)
        want[own] = 2.5
        assert np.array_equal(dev.read(s_ptr, 3), want), me
        seen_empty += len(own) == 0
        assert sub.algorithmic_bytes(3) == (12 + 28 + 8 + 8) * len(own) if len(own) else sub.algorithmic_bytes(3) == 4
    assert seen_empty == 2


def test_aggregate_sums_obeys_its_stream(schwz, torch_cuda):
    """On a non-default stream held shut by a delay, beside a default stream that runs: the calls return while the gate
    is shut and s equals the default-stream run bit for bit (stream_rig.py: a launch on another stream reads the
    poison the input still holds, or its result is overwritten)."""
    torch = torch_cuda
    shape, P = (12, 12, 12), 3
    n_all = shape[0] * shape[1] * shape[2]
    agg = boxes(shape, (4, 4, 2))
    first = [0, 18, 36, 54]

    def body(r):
        prob = r.hold(schwz.Problem.laplacian(3, *shape))
        fr = schwz.partition_regular(n_all, P)
        sds = [r.hold(schwz.Subdomain(prob, P, me, 2, fr)) for me in range(P)]
        coarse = r.hold(schwz.Coarse(np.eye(54)))
        d_v = []
        for me, sd in enumerate(sds):
            sd.to_device(np.ones(sd.local_size_x), precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=4)
            sd.coarse_set_aggregates(agg[sd.local_to_global], first[me], 18, 54)
            # the first use builds and uploads the tables (it waits for the stream, once): before the gate
            sd.aggregate_sums(coarse, r.hold(torch.zeros(sd.local_size_x, dtype=torch.float64, device="cuda")).data_ptr())
            d_v.append(r.input(np.random.default_rng(90 + me).standard_normal(sd.local_size_x)))
        idx = r.hold(torch.arange(54, dtype=torch.int32, device="cuda"))
        r.arm()
        for me, sd in enumerate(sds):
            r.call(sd.aggregate_sums, coarse, d_v[me].data_ptr(), stream=r.handle)
        p, cnt = coarse.vector(0)
        t = r.output(cnt)
        schwz.gather(cnt, idx.data_ptr(), p, t.data_ptr(), stream=r.handle)
        r.snap(t)
        return []

    snaps, _ = rig.both(torch, body, "aggregate sums")
    assert np.isfinite(snaps[0]).all() and np.abs(snaps[0]).min() > 0
