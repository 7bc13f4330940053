"""The device steps of one RAS iteration on general matrices, each against a longdouble restatement at a derived bound
(hp_reference.py: residual_bound per row, norm_sq_bound for the sums of squares; Higham section 3.1, valid for any
summation order, nothing measured on a kernel), and the exchange primitives bit for bit.

  norms      schwz_ras_local_residual (b~, all rows), schwz_ras_true_residual_sq (rhs, rows below local_size: the one
             caller that puts row_limit inside the matrix) and the check norm of schwz_ras_check_and_solve_launch
             (the dual residual: x2 = x~, x = y), per matrix coding and spmv_variant.  An off-by-one in a kernel's
             `row < a.row_limit` moves the sum by one row's square: every case asserts on the CPU, before it touches
             the GPU, that the squares of the rows at the limit are more than four times the bound.
  interface  b~ = rhs - A_Gamma x~ on the overlap rows (row-wise, badly scaled rows included), rhs bits below them.
  exchange   pack / unpack, their fp32 forms, the per-neighbour forms and pack_early: exact.

What the check-norm case writes into y: the fused launch forms the second product (A x~ beside A y) only in tiles
that reach the overlap -- rows or columns at or past local_size (csr_set_dual_split); elsewhere it takes y's
residual for x~'s, because between a restriction and the next solve y IS x~ on the interior rows.  A y that differs
from x~ there is outside that contract (the check norm then mixes the two vectors: seen here with a fully random
y, 0.14 rho^2 off), so the case writes another random vector on the overlap rows and x~ on the interior rows.
On a subdomain without overlap (P = 1) there is no second vector at all: a write into y stands for x~ in the next
check residual (subdomain.hip, "where y lives"; pinned by test_gpu_cg_fixed_part.py), so there the random vector
goes into x~ as well."""
import ctypes as C
import os

import numpy as np
import pytest

import cg_child as cc
import hp_reference as hp

pytestmark = pytest.mark.gpu

VARIANTS = (0, 6, 7, 8, 9)
PATTERN = {"SCHWZ_SPMV_PAIR": "0", "SCHWZ_SPMV_PATTERN": "2", "SCHWZ_SPMV_DICT": "0"}
CODINGS = {"plain": (cc.PLAIN, (0,)), "dictionary": (cc.DICT, (1,)), "patterns": (PATTERN, (2,)),
           "pairs": (cc.PAIRS, (2, 3))}      # (switches at upload, schwz_csr_format of the local matrix)
K = 6                                        # inner iterations of the pack_early case


def global_case(name):
    """(rp, col, val, P, first_row or "graph" or None, exponents of the row scaling or None), seeded by name."""
    rng = np.random.default_rng(sum(name.encode()) + 2000)
    if name.startswith("band_p"):
        return hp.sym_band_matrix(1500, 6, 40, rng) + (int(name[6:]), None, None)
    if name == "nonsym_band_p3":            # the SPD band with its upper triangle halved: still diagonally dominant
        rp, col, val = hp.sym_band_matrix(1500, 6, 40, rng)
        val = np.where(col > np.repeat(np.arange(1500), np.diff(rp)), 0.5 * val, val)
        return rp, col, val, 3, None, None
    if name == "scaled_band_p3":
        rp, col, val = hp.sym_band_matrix(1500, 6, 40, rng, spd=False)
        val, s, _ = hp.rescale_rows_cols(rp, col, val, rng)
        return rp, col, val, 3, None, s
    if name == "ani4_graph_p3":
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ani4_crop.npz"))
        return g["rp"], g["col"], g["val"], 3, "graph", None
    if name == "arrow_p2":
        # (an even split would leave subdomain 1 a row 0 of 1500-odd entries: 500 | 2500 gives both a long one)
        return hp.arrow_matrix(3000, rng) + (2, np.array([0, 500, 3000]), None)
    if name == "window2049_p1":
        return hp.window2049_square(rng) + (1, None, None)
    if name.startswith("band7_at_"):        # rows of at most 7 entries: tiles of 256 rows; local_size = the number
        rp, col, val = hp.sym_band_matrix(1500, 3, 3, rng)
        assert np.diff(rp).max() <= 7
        L = int(name[9:]) if name[9:] != "last" else 1499
        return rp, col, val, 2, np.array([0, L, 1500]), None
    if name == "ragged32_inside_a_tile":    # tiles limited by their entries; local_size inside the third one
        rp, col, val = hp.sym_band_matrix(1501, 14, 400, rng, spd=False)
        t = hp.tiles_of(rp)
        assert np.diff(t)[:4].max() < 256
        return rp, col, val, 2, np.array([0, (t[2] + t[3]) // 2, 1501]), None
    raise KeyError(name)


class StepRig:
    """The subdomains `which` of one partition on the device, x~ (interior, overlap and halo) and the rhs random."""

    def __init__(self, schwz, torch, name, env, variant=0, which=None, maxit=0, connect=True, device_kw=None):
        """device_kw: further options of Subdomain.to_device (the local solver of test_gpu_streams.py)."""
        self.schwz, self.torch = schwz, torch
        rp, col, val, P, fr, s = global_case(name)
        self.P = P
        prob = schwz.Problem.from_csr(rp, col, val)
        if isinstance(fr, str):
            prob, _, fr = prob.permute(prob.partition_graph(P), P)
        elif fr is None:
            fr = schwz.partition_regular(prob.N, P)
        self.prob, self.N = prob, prob.N
        self.which = list(range(P)) if which is None else list(which)
        self.sds = {me: schwz.Subdomain(prob, P, me, 2, fr) for me in self.which}
        if connect and P > 1:
            assert len(self.which) == P
            lists = schwz.InProcessComm(P).handshake({me: sd.get_lists() for me, sd in self.sds.items()})
            for me, lst in lists.items():
                for q, ids in lst:
                    self.sds[me].add_put_list(q, ids)
        rng = np.random.default_rng(sum(name.encode()) + 3000)
        rhs = rng.standard_normal(self.N)
        self.rhs_global = rhs if s is None else np.ldexp(rhs, s)
        self.rhs, self.x, self.idx, self.l2g = {}, {}, {}, {}
        with cc.upload_env(env):
            for me, sd in self.sds.items():
                self.l2g[me] = sd.local_to_global
                self.rhs[me] = self.rhs_global[self.l2g[me][:sd.local_size_x]].copy()
                sd.to_device(self.rhs[me], precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=maxit,
                             spmv_variant=variant, **(device_kw or {}))
                nx = sd.local_size_x + sd.halo_size
                self.idx[me] = torch.arange(max(nx, 1), dtype=torch.int32, device="cuda")
                self.x[me] = np.random.default_rng(4000 + me).standard_normal(nx)
                self.put(me, 0, self.x[me])

    def format(self, me):
        h = C.c_void_p()
        self.schwz.capi.check(self.schwz.capi.lib.schwz_ras_local_csr(self.sds[me].h, C.byref(h)))
        return int(self.schwz.capi.lib.schwz_csr_format(h))

    def get(self, me, which_vec):
        p, cnt = self.sds[me].vector(which_vec)
        t = self.torch.empty(max(cnt, 1), dtype=self.torch.float64, device="cuda")
        self.schwz.gather(cnt, self.idx[me].data_ptr(), p, t.data_ptr())
        self.torch.cuda.synchronize()
        return t.cpu().numpy()[:cnt]

    def put(self, me, which_vec, a):
        p, cnt = self.sds[me].vector(which_vec)
        assert len(a) == cnt
        t = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        self.schwz.gather(cnt, self.idx[me].data_ptr(), t.data_ptr(), p)
        self.torch.cuda.synchronize()

    def local_ids(self, me, global_ids):
        inv = np.full(self.N, -1, dtype=np.int64)
        inv[self.l2g[me]] = np.arange(len(self.l2g[me]))
        out = inv[np.asarray(global_ids, dtype=np.int64)]
        assert (out >= 0).all()
        return out

    def exchange_and_update(self):
        """One synchronous halo exchange through torch buffers, then b~."""
        torch, bufs = self.torch, {}
        send = {me: torch.zeros(max(sd.num_send, 1), dtype=torch.float64, device="cuda") for me, sd in self.sds.items()}
        for me, sd in self.sds.items():
            sd.pack(send[me].data_ptr())
            off = sd.send_offsets()
            for k, (q, _) in enumerate(sd.put_lists()):
                bufs[(me, q)] = send[me][off[k]:off[k + 1]]
        torch.cuda.synchronize()
        for me, sd in self.sds.items():
            recv = torch.zeros(max(sd.num_recv, 1), dtype=torch.float64, device="cuda")
            off = sd.recv_offsets()
            for k, (p, _) in enumerate(sd.get_lists()):
                recv[off[k]:off[k + 1]].copy_(bufs[(p, me)])
            sd.unpack(recv.data_ptr())
            sd.update_boundary()
        torch.cuda.synchronize()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


# ---- norms ---------------------------------------------------------------------------------------------------------

_norm_refs = {}


def norm_reference(rig, name):
    """Per subdomain: the local matrix, and the longdouble residuals, their row-wise bounds and the bounds of the
    three sums, with the discrimination condition asserted.  Once per partition: coding and variant change no input
    (b~ is read back from the first rig and compared bit for bit in the later ones)."""
    if name in _norm_refs:
        return _norm_refs[name]
    hp.require_extended_precision()
    out = {}
    for me, sd in rig.sds.items():
        n, L = sd.local_size_x, sd.local_size
        rp, col, val = sd.local_matrix()
        x = rig.x[me][:n]
        y = np.random.default_rng(5000 + me).standard_normal(n)
        if sd.overlap_size > 0:
            y[:L] = x[:L]      # the fused launch's contract (see the module docstring): y is x~ on the interior rows
        bt = rig.get(me, 1)
        ref = dict(rp=rp, y=y, bt=bt)
        for key, (vec, b, rows, root) in dict(local=(x, bt, n, True), true=(x, rig.rhs[me], L, False),
                                              start=(y, bt, n, True)).items():
            r = hp.residual(rp, col, val, vec, b)
            e = hp.residual_bound(rp, col, val, vec, b)
            B = hp.norm_sq_bound(r, e, rows, root=root)
            rho2 = np.sum(r[:rows] * r[:rows])
            # one row more or one row less must show: r_{L-1}^2 > 4 B and r_L^2 > 4 B
            assert r[rows - 1] ** 2 > 4 * B, (name, me, key)
            assert rows == n or r[rows] ** 2 > 4 * B, (name, me, key)
            ref[key] = (rho2, B)
        out[me] = ref
    _norm_refs[name] = out
    return out


def run_norm_case(schwz, torch, name, coding, which=None, long_rows=0, branch=None):
    env, formats = CODINGS[coding]
    worst = {"local": 0.0, "true": 0.0, "check": 0.0, "start": 0.0}
    for variant in VARIANTS:
        rig = StepRig(schwz, torch, name, env, variant, which=which, connect=which is None)
        if rig.P > 1 and which is None:
            rig.exchange_and_update()          # b~ differs from the rhs on the overlap rows, x~ holds the neighbours' values
            for me in rig.sds:
                rig.x[me] = rig.get(me, 0)
        refs = norm_reference(rig, name)
        for me, sd in rig.sds.items():
            ref = refs[me]
            assert rig.format(me) in formats, (name, coding, me, rig.format(me))
            assert np.array_equal(bits(rig.get(me, 1)), bits(ref["bt"]))
            lens = np.diff(ref["rp"])
            assert (lens > 2048).sum() >= long_rows, lens.max()
            if branch:
                assert branch in hp.tile_branches(ref["rp"])
            n = sd.local_size_x

            def ratio(got_sq, key):
                rho2, B = ref[key]
                return float(abs(hp.LD(got_sq) - rho2) / B)

            tag = "%s %s variant %d subdomain %d" % (name, coding, variant, me)
            q = ratio(hp.LD(sd.local_residual()) ** 2, "local")
            assert q <= 1.0, (tag, "local_residual", q)
            worst["local"] = max(worst["local"], q)
            if sd.local_size > 0:
                q = ratio(sd.true_residual_sq(), "true")
                assert q <= 1.0, (tag, "true_residual_sq with row_limit %d of %d" % (sd.local_size, n), q)
                worst["true"] = max(worst["true"], q)
            # the fused launch with no iteration: the check norm is x~'s, the start residual y's, y is not touched
            if sd.overlap_size == 0:
                rig.put(me, 0, np.concatenate([ref["y"], rig.x[me][n:]]))     # no overlap: y stands for x~
            rig.put(me, 2, ref["y"])
            x_before = rig.get(me, 0)
            sd.check_and_solve_launch()
            check = sd.local_residual_wait()
            torch.cuda.synchronize()
            iters, start = sd.last_inner_stats()
            assert iters == 0
            q = ratio(hp.LD(check) ** 2, "start" if sd.overlap_size == 0 else "local")
            assert q <= 1.0, (tag, "check norm", q)
            worst["check"] = max(worst["check"], q)
            q = ratio(hp.LD(start) ** 2, "start")
            assert q <= 1.0, (tag, "start residual norm of last_inner_stats", q)
            worst["start"] = max(worst["start"], q)
            assert np.array_equal(bits(rig.get(me, 2)), bits(ref["y"])), (tag, "y changed")
            assert np.array_equal(bits(rig.get(me, 0)), bits(x_before)), (tag, "x~ changed")
        del rig
    print("\nnorms %-24s %-10s max error / bound: local_residual %.1e true_residual_sq %.1e check %.1e start %.1e"
          % (name, coding, worst["local"], worst["true"], worst["check"], worst["start"]))


@pytest.mark.parametrize("coding", sorted(CODINGS))
@pytest.mark.parametrize("name", ["band_p1", "band_p2", "band_p3", "ani4_graph_p3"])
def test_norms_on_general_matrices(schwz, torch_cuda, name, coding):
    run_norm_case(schwz, torch_cuda, name, coding)


@pytest.mark.parametrize("coding", sorted(CODINGS))
def test_norms_with_a_long_row_in_every_local_matrix(schwz, torch_cuda, coding):
    """Arrow matrix: both local matrices hold a row of more than 2048 entries, so the fused modes (kSpmvResidNorm,
    kSpmvResidDual) run the workgroup-reduction branch."""
    run_norm_case(schwz, torch_cuda, "arrow_p2", coding, long_rows=1, branch="c")


@pytest.mark.parametrize("coding", sorted(CODINGS))
def test_norms_on_the_unaligned_staging_branch(schwz, torch_cuda, coding):
    run_norm_case(schwz, torch_cuda, "window2049_p1", coding, branch="b")


@pytest.mark.parametrize("coding", sorted(CODINGS))
@pytest.mark.parametrize("name", ["band7_at_1", "band7_at_255", "band7_at_256", "band7_at_257", "band7_at_last",
                                  "ragged32_inside_a_tile"])
def test_true_residual_row_limit_positions(schwz, torch_cuda, name, coding):
    """local_size at 1, next to and on a tile boundary (256), one below local_size_x, and inside a tile that is limited
    by its entries: subdomain 0 of two, placed through first_row."""
    rig = StepRig(schwz, torch_cuda, name, cc.PLAIN, which=[0], connect=False)
    sd = rig.sds[0]
    t = hp.tiles_of(sd.local_matrix()[0])
    if name == "band7_at_last":
        assert sd.local_size == sd.local_size_x - 1
    elif name.startswith("band7"):
        assert sd.local_size == int(name[9:]) and sd.local_size_x > sd.local_size
        assert sd.local_size_x <= 256 or t[1] == 256         # 256 is a tile boundary wherever the matrix reaches it
    else:
        k = int(np.searchsorted(t, sd.local_size, side="right")) - 1
        assert t[k] < sd.local_size < t[k + 1] and t[k + 1] - t[k] < 256 and k + 2 < len(t)
    del rig
    run_norm_case(schwz, torch_cuda, name, coding, which=[0])


# ---- interface update ----------------------------------------------------------------------------------------------

def check_interface(rig, name):
    worst = 0.0
    for me, sd in rig.sds.items():
        n, L = sd.local_size_x, sd.local_size
        assert sd.overlap_size > 0 and sd.nnz_interface > 0
        irp, icol, ival = sd.interface_matrix()
        assert irp[L] == 0                                       # interior rows have no interface entries
        x = rig.get(me, 0)
        xg = np.zeros(rig.N)
        xg[rig.l2g[me]] = x
        r = hp.residual(irp, icol, ival, xg, rig.rhs[me])
        e = hp.residual_bound(irp, icol, ival, xg, rig.rhs[me])
        bt = rig.get(me, 1)
        assert np.array_equal(bits(bt[:L]), bits(rig.rhs[me][:L])), (name, me, "b~ below local_size")
        err = np.abs(bt[L:].astype(hp.LD) - r[L:])
        q = err / e[L:]
        i = int(np.argmax(q))
        assert q[i] <= 1.0, ("%s subdomain %d: overlap row %d (%d interface entries) is %.3g times its bound off: "
                             "got %r, reference %r" % (name, me, i, irp[L + i + 1] - irp[L + i], float(q[i]), bt[L + i],
                                                       r[L + i]))
        assert (np.abs(bt[L:] - rig.rhs[me][L:]) > 0).any()      # (the update did something)
        worst = max(worst, float(q[i]))
    return worst


@pytest.mark.parametrize("name", ["scaled_band_p3", "ani4_graph_p3"])
def test_interface_update_row_by_row(schwz, torch_cuda, name):
    rig = StepRig(schwz, torch_cuda, name, {})
    rig.exchange_and_update()
    print("\ninterface %-16s max error / bound %.3f" % (name, check_interface(rig, name)))


def test_interface_update_and_fp32_halo_past_the_launch_cap(schwz, torch_cuda):
    """1024 x 1024 x 4 in two slabs: 2^20 overlap rows and as many entries to send, past the 2048 x 256 threads of one
    launch: the grid-stride form of interface_update_kernel, gather_f32_kernel and scatter_f32_kernel."""
    torch = torch_cuda
    prob = schwz.Problem.laplacian(3, 1024, 1024, 4)
    P = 2
    fr = schwz.partition_regular(prob.N, P)
    sds = [schwz.Subdomain(prob, P, me, 2, fr) for me in range(P)]
    for me, lst in schwz.InProcessComm(P).handshake({me: sd.get_lists() for me, sd in enumerate(sds)}).items():
        for q, ids in lst:
            sds[me].add_put_list(q, ids)
    sd = sds[0]
    assert sd.overlap_size > 524288 and sd.num_send > 524288 and sd.num_recv > 524288
    rng = np.random.default_rng(9)
    n, nx = sd.local_size_x, sd.local_size_x + sd.halo_size
    rhs = rng.standard_normal(n)
    sd.to_device(rhs, precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=0)
    x = rng.standard_normal(nx)
    p, cnt = sd.vector(0)
    assert cnt == nx
    d_x = torch.from_numpy(x).cuda()
    idx = torch.arange(nx, dtype=torch.int32, device="cuda")
    schwz.gather(nx, idx.data_ptr(), d_x.data_ptr(), p)
    l2g = sd.local_to_global
    inv = np.full(prob.N, -1, dtype=np.int64)
    inv[l2g] = np.arange(nx)
    put_ids = np.concatenate([inv[ids] for _, ids in sd.put_lists()])
    get_ids = np.concatenate([inv[ids] for _, ids in sd.get_lists()])
    # fp32 pack and unpack
    send = torch.zeros(sd.num_send, dtype=torch.float32, device="cuda")
    sd.pack_f32(send.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(send.cpu().numpy()), bits(x[put_ids].astype(np.float32))), "pack_f32"
    recv = rng.standard_normal(sd.num_recv).astype(np.float32)
    d_recv = torch.from_numpy(recv).cuda()
    sd.unpack_f32(d_recv.data_ptr())
    x[get_ids] = recv.astype(np.float64)
    # interface update
    sd.update_boundary()
    t = torch.empty(n, dtype=torch.float64, device="cuda")
    schwz.gather(n, idx.data_ptr(), sd.vector(1)[0], t.data_ptr())
    got_x = torch.empty(nx, dtype=torch.float64, device="cuda")
    schwz.gather(nx, idx.data_ptr(), p, got_x.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(got_x.cpu().numpy()), bits(x))
    bt, L = t.cpu().numpy(), sd.local_size
    irp, icol, ival = sd.interface_matrix()
    xg = np.zeros(prob.N)
    xg[l2g] = x
    hp.require_extended_precision()
    r = hp.residual(irp, icol, ival, xg, rhs)
    e = hp.residual_bound(irp, icol, ival, xg, rhs)
    assert np.array_equal(bits(bt[:L]), bits(rhs[:L]))
    q = np.abs(bt[L:].astype(hp.LD) - r[L:]) / e[L:]
    assert q.max() <= 1.0, (int(np.argmax(q)), float(q.max()))
    assert (np.diff(irp)[L:] > 0).all()
    print("\ninterface 1024x1024x4     overlap rows %d, sent %d: max error / bound %.3f" % (sd.overlap_size, sd.num_send, float(q.max())))


# ---- exchange primitives, exact ------------------------------------------------------------------------------------

SPECIAL = np.array([-0.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 3.5e38, -1e300, 1e-40, 2.0 ** -150, 0.75, -1234.5678,
                    2.0 ** -126, -(2.0 ** -127), 3.0e-39, 1.0000001, -3.4028235677973366e38])
TINY = 2.0 ** -126      # the smallest normal float32


def special_vector(n, seed):
    """Every entry of SPECIAL many times over, mixed with ordinary values: whichever ids a put list holds, it meets
    them all."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n)
    at = rng.random(n) < 0.6
    v[at] = SPECIAL[rng.integers(0, len(SPECIAL), int(at.sum()))]
    return v


def check_f32(got, src, what):
    """got = float32(src) bit for bit where the result is normal, zero, or overflows; below 2^-126 within 2^-126 of src
    (gradual underflow and flush to zero both pass; which one the device does is printed and stated in DESIGN)."""
    with np.errstate(over="ignore"):
        exp = src.astype(np.float32)
    small = (np.abs(src) < TINY) & (src != 0)
    assert np.array_equal(bits(got[~small]), bits(exp[~small])), what
    assert (np.abs(got[small].astype(np.float64) - src[small]) <= TINY).all(), what
    flushed = small & (got == 0) & (exp != 0)
    return int(small.sum()), int(flushed.sum())


def test_pack_and_unpack_are_exact(schwz, torch_cuda):
    torch = torch_cuda
    rig = StepRig(schwz, torch, "band_p3", {})
    small = flushed = 0
    for me, sd in rig.sds.items():
        nx = sd.local_size_x + sd.halo_size
        x = special_vector(nx, 60 + me)
        put_ids = rig.local_ids(me, np.concatenate([ids for _, ids in sd.put_lists()]))
        first = put_ids[np.sort(np.unique(put_ids, return_index=True)[1])][:2 * len(SPECIAL)]
        assert len(first) >= len(SPECIAL)
        x[first] = np.resize(SPECIAL, len(first))         # whatever the random mix put there: every value is sent
        rig.put(me, 0, x)
        get_ids = rig.local_ids(me, np.concatenate([ids for _, ids in sd.get_lists()]))
        assert len(np.unique(get_ids)) == len(get_ids) == sd.num_recv and len(put_ids) == sd.num_send
        for v in SPECIAL:
            assert (bits(x[put_ids]) == bits(np.array([v]))[0]).any()
        # ---- pack, pack_f32, pack_neighbor
        send = torch.zeros(sd.num_send, dtype=torch.float64, device="cuda")
        send32 = torch.zeros(sd.num_send, dtype=torch.float32, device="cuda")
        sd.pack(send.data_ptr())
        sd.pack_f32(send32.data_ptr())
        torch.cuda.synchronize()
        packed, packed32 = send.cpu().numpy(), send32.cpu().numpy()
        assert np.array_equal(bits(packed), bits(x[put_ids])), (me, "pack")
        s, f = check_f32(packed32, x[put_ids], (me, "pack_f32"))
        small, flushed = small + s, flushed + f
        assert np.isinf(packed32[np.abs(x[put_ids]) > 3.4028235677973366e38]).all()
        off = sd.send_offsets()
        assert sd.num_neighbors_out == (1 if me in (0, rig.P - 1) else 2)
        for k in range(sd.num_neighbors_out):
            cnt = off[k + 1] - off[k]
            one = torch.full((cnt + 2,), 7.0, dtype=torch.float64, device="cuda")
            one32 = torch.full((cnt + 2,), 7.0, dtype=torch.float32, device="cuda")
            sd.pack_neighbor(k, one.data_ptr() + 8, single=False)
            sd.pack_neighbor(k, one32.data_ptr() + 4, single=True)
            torch.cuda.synchronize()
            one, one32 = one.cpu().numpy(), one32.cpu().numpy()
            assert np.array_equal(bits(one[1:-1]), bits(packed[off[k]:off[k + 1]])), (me, k, "pack_neighbor")
            assert np.array_equal(bits(one32[1:-1]), bits(packed32[off[k]:off[k + 1]])), (me, k, "pack_neighbor fp32")
            assert one[0] == 7.0 and one[-1] == 7.0 and one32[0] == 7.0 and one32[-1] == 7.0
        # ---- unpack, unpack_f32, unpack_neighbor
        roff = sd.recv_offsets()
        recv = special_vector(sd.num_recv, 70 + me)
        with np.errstate(over="ignore"):
            recv32 = special_vector(sd.num_recv, 80 + me).astype(np.float32)
        d_recv, d_recv32 = torch.from_numpy(recv).cuda(), torch.from_numpy(recv32).cuda()
        for single in (False, True):
            src = recv32.astype(np.float64) if single else recv
            d_src, esize = (d_recv32, 4) if single else (d_recv, 8)
            want = x.copy()
            want[get_ids] = src
            rig.put(me, 0, x)
            (sd.unpack_f32 if single else sd.unpack)(d_src.data_ptr())
            assert np.array_equal(bits(rig.get(me, 0)), bits(want)), (me, single, "unpack")
            rig.put(me, 0, x)
            for k in range(sd.num_neighbors_in):
                sd.unpack_neighbor(k, d_src.data_ptr() + esize * roff[k], single=single)
                part = x.copy()
                part[get_ids[:roff[k + 1]]] = src[:roff[k + 1]]
                assert np.array_equal(bits(rig.get(me, 0)), bits(part)), (me, single, k, "unpack_neighbor")
            assert np.array_equal(bits(rig.get(me, 0)), bits(want))
    assert small > 0
    print("\nexchange: %d packed fp32 values below 2^-126, %d of them flushed to zero (%s)"
          % (small, flushed, "flush to zero" if flushed == small else ("gradual underflow" if flushed == 0 else "mixed")))


def test_pack_early_equals_pack_after_restrict(schwz, torch_cuda):
    torch = torch_cuda
    rig = StepRig(schwz, torch, "band_p3", {}, maxit=K)
    rig.exchange_and_update()
    for me, sd in rig.sds.items():
        assert sd.early_pack_ok() == 1
        for single in (False, True):
            dt = torch.float32 if single else torch.float64
            early = torch.zeros(sd.num_send, dtype=dt, device="cuda")
            late = torch.zeros(sd.num_send, dtype=dt, device="cuda")
            sd.check_and_solve_launch()
            sd.pack_early(early.data_ptr(), single=single)
            torch.cuda.synchronize()
            assert sd.last_inner_stats()[0] == K
            sd.restrict()
            (sd.pack_f32 if single else sd.pack)(late.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(bits(early.cpu().numpy()), bits(late.cpu().numpy())), (me, single)
            assert early.abs().max() > 0
