"""The stream contract of include/schwz_hip.h ("all device entry points are asynchronous on `stream`") on streams
other than the legacy default stream, which is the only one the rest of the suite ever passes.

Every case runs its calls twice through stream_rig.py: on the default stream with fresh objects (the reference), and
"gated" on a non-blocking stream S that a delay holds shut while the calls are issued, with every input poisoned
until the gate has passed (see stream_rig.py).  The two runs must agree bit for bit.  So that "identical to the
default stream" cannot mean "identically wrong", the reference run of each family is held once to the
extended-precision restatement and the bound its own module uses (imported from there, not copied).

  (a) gather / scatter and their typed forms, Csr.spmv per coding and variant
  (b) Pcg: graph replays, the deferred x with its postponed tail, tolerance stops (the polling path), general
      preconditioners, a cached graph replayed on another stream than it was recorded for
  (c) PcgF32, Chebyshev, Gmres, Bicgstab
  (d) Trs: one-workgroup, flag, flag-wave and level-plan (graph) solves, Jacobi sweeps
  (e) the device steps of a RAS iteration, per local solver, with the early pack and the norm on second streams
  (f) the Python host with a non-default current stream
  (g) creation calls take no stream: they are complete on return
  (h) independent objects on several streams at once
  and the proof that the rig fails when a launch goes to the wrong stream.

Calls that read back on the host (want_stats=True solves, solves with a tolerance -- the host polls the solver's
state --, GMRES past its second cycle and BiCGSTAB past its second polling batch, local_residual_wait,
last_inner_stats, true_residual_sq, get_interior) synchronise by contract: for them only the values are compared, and
so for whatever a case calls after its first read-back (the second outer iteration of (e)).  Every other call is
asserted to return while the gate is still shut.  Every stream here is non-blocking: what the header says about blocking
streams is contract, not something these cases establish.

Skips: no extended precision (hp.require_extended_precision), nothing else."""
import ctypes as C
import time

import numpy as np
import pytest

import cg_child as cc
import hp_bicgstab
import hp_chebyshev
import hp_reference as hp
import stream_rig as rig
import test_gpu_cg as tcg
import test_gpu_mixed as tgm
import test_gpu_ras_steps as steps
import test_gpu_spmv_modes as tsm
import test_gpu_trs as ttrs

pytestmark = pytest.mark.gpu

LD = np.longdouble
VARIANTS = (0, 6, 7, 8, 9)
D2 = {"SCHWZ_CG_DEFERX": "2"}
_T0 = [None]


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The host-side durations DELAY_MS is derived from, and the wall time of the module (profiles/r17_stream_contract.txt)."""
    _T0[0] = time.time()
    yield
    whole = [e for e in rig.CALL_LOG if e[0].startswith("the first outer")]
    top = sorted((e for e in rig.CALL_LOG if e not in whole), key=lambda e: -e[1])[:8]
    print("\nstream contract: %d default-stream calls timed; the longest on the host:" % (len(rig.CALL_LOG) - len(whole)))
    for name, ms in top + whole:
        print("  %8.3f ms  %s" % (ms, name))
    print("stream contract: delay %.0f ms (%g sleep units per ms); module wall time %.1f s"
          % (rig.DELAY_MS, rig._rate.get("rate", float("nan")), time.time() - _T0[0]))


def _lap(oracle, shape):
    return cc.laplacian(oracle, shape)


# ---- (a) stand-alone kernels -------------------------------------------------------------------------------------------

def _op_ref(op, capi, into, frm):
    if op == capi.OP_COPY:
        return frm.copy()
    if op == capi.OP_ADD:
        return frm + into
    if op == capi.OP_DIFF:
        return frm - into
    s = frm + into
    if into.dtype.kind == "f":
        return (s / np.array(2, dtype=into.dtype)).astype(into.dtype)
    return (np.sign(s) * (np.abs(s) // 2)).astype(into.dtype)


def _gather_scatter_body(schwz, n, m, idx, frm_g, into_g, frm_s, into_s, op):
    def body(r):
        d_idx = r.input(idx, index=True)
        d_fg, d_fs, d_is = r.input(frm_g), r.input(frm_s), r.input(into_s)
        d_ig = r.output(n) if op == schwz.capi.OP_COPY else r.input(into_g)
        r.arm()
        r.call(schwz.gather, n, d_idx.data_ptr(), d_fg.data_ptr(), d_ig.data_ptr(), op, stream=r.handle)
        r.call(schwz.scatter, n, d_idx.data_ptr(), d_fs.data_ptr(), d_is.data_ptr(), op, stream=r.handle)
        r.snap(d_ig)
        r.snap(d_is)
    return body


def _gather_scatter_inputs(n, dtype=np.float64, itype=np.int32):
    rng = np.random.default_rng(n)
    m = n + 37
    idx = rng.permutation(m)[:n].astype(itype)               # distinct targets: the scatter has no collisions
    mk = lambda k, s: (rng.standard_normal(k) * s).astype(dtype)   # noqa: E731
    return m, idx, mk(m, 100), mk(n, 10), mk(n, 100), mk(m, 10)


@pytest.mark.parametrize("n", [1000, 524289])
@pytest.mark.parametrize("op", ["COPY", "ADD", "DIFF", "AVG"])
def test_gather_and_scatter_on_a_stream(schwz, torch_cuda, op, n):
    """n = 524 289: one past the 2048 x 256 threads of a launch, the grid-stride form."""
    code = getattr(schwz.capi, "OP_" + op)
    m, idx, frm_g, into_g, frm_s, into_s = _gather_scatter_inputs(n)
    (g, s), _ = rig.both(torch_cuda, _gather_scatter_body(schwz, n, m, idx, frm_g, into_g, frm_s, into_s, code),
                         "gather/scatter %s n=%d" % (op, n))
    assert np.array_equal(g[:n], _op_ref(code, schwz.capi, into_g, frm_g[idx]))
    want = into_s.copy()
    want[idx] = _op_ref(code, schwz.capi, into_s[idx], frm_s)
    assert np.array_equal(s, want)


@pytest.mark.parametrize("vt,it", [("float32", "int64"), ("int64", "int32")])
def test_typed_gather_and_scatter_on_a_stream(schwz, torch_cuda, vt, it):
    n = 524289
    lib, check, capi = schwz.capi.lib, schwz.capi.check, schwz.capi
    vcode = {"float32": 0, "float64": 1, "int32": 2, "int64": 3}[vt]
    icode = {"int32": 0, "int64": 1}[it]
    m, idx, frm_g, into_g, frm_s, into_s = _gather_scatter_inputs(n, vt, it)
    op = capi.OP_ADD

    def body(r):
        d_idx = r.input(idx, index=True)
        d_fg, d_ig, d_fs, d_is = r.input(frm_g), r.input(into_g), r.input(frm_s), r.input(into_s)
        r.arm()
        st = C.c_void_p(r.handle) if r.handle else None
        r.call(lambda: check(lib.schwz_gather_typed(n, d_idx.data_ptr(), icode, d_fg.data_ptr(), d_ig.data_ptr(), vcode,
                                                    op, st)), label="schwz_gather_typed")
        r.call(lambda: check(lib.schwz_scatter_typed(n, d_idx.data_ptr(), icode, d_fs.data_ptr(), d_is.data_ptr(), vcode,
                                                     op, st)), label="schwz_scatter_typed")
        r.snap(d_ig)
        r.snap(d_is)
    (g, s), _ = rig.both(torch_cuda, body, "typed %s/%s" % (vt, it))
    assert np.array_equal(g, _op_ref(op, capi, into_g, frm_g[idx]))
    want = into_s.copy()
    want[idx] = _op_ref(op, capi, into_s[idx], frm_s)
    assert np.array_equal(s, want)


UPLOADS = {"pairs": ((24, 20, 17), cc.PAIRS, 3), "dictionary": ((24, 20, 17), cc.DICT, 1),
           "plain": ((24, 20, 17), cc.PLAIN, 0), "walk": ((256, 4, 12), cc.SMALL_WALK, 3)}


@pytest.mark.parametrize("upload", list(UPLOADS))
def test_spmv_on_a_stream(schwz, oracle, torch_cuda, upload):
    """y = alpha A x + beta y with alpha, beta != 0 (y is an input), every variant of the product library."""
    hp.require_extended_precision()
    shape, env, fmt = UPLOADS[upload]
    rp, col, val = _lap(oracle, shape)
    n = len(rp) - 1
    rng = np.random.default_rng(n)
    x, y0 = rng.standard_normal(n), rng.standard_normal(n)
    alpha, beta = 0.5, -2.0

    def body(r):
        with cc.upload_env(env):
            A = r.hold(schwz.Csr(rp, col, val))
        assert A.format() == fmt and (A.sweep_slots() > 0) == (upload == "walk")
        d_x = r.input(x)
        ys = [r.input(y0) for _ in VARIANTS]
        r.arm()
        for v, d_y in zip(VARIANTS, ys):
            r.call(A.spmv, d_x.data_ptr(), d_y.data_ptr(), alpha, beta, variant=v, stream=r.handle)
        for d_y in ys:
            r.snap(d_y)
    got, _ = rig.both(torch_cuda, body, "spmv " + upload)
    ref = hp.axpby(rp, col, val, x, alpha, beta, y0)
    bound = hp.axpby_bound(rp, col, val, x, alpha, beta, y0)
    for v, y in zip(VARIANTS, got):
        q, row = tsm.worst_row(y, ref, bound)
        assert q <= 1.0, (upload, v, row, q)


# ---- (b) Pcg -----------------------------------------------------------------------------------------------------------

def _pcg_body(schwz, mat, env_up, solves, want_stats, precond=1, bs=1, **kw):
    """solves: (b, x0, rtol, iters, switches of the solve), one after the other on one object and one stream."""
    def body(r):
        with cc.upload_env(env_up):
            A = r.hold(schwz.Csr(*mat))
            cg = r.hold(schwz.Pcg(A, precond, bs, **kw))
        bufs = [(r.input(s[0]), r.input(s[1])) for s in solves]
        r.arm()
        host = []
        for (d_b, d_x), (_, _, rtol, iters, env) in zip(bufs, solves):
            with cc.upload_env(env):
                out = r.call(cg.solve, d_b.data_ptr(), d_x.data_ptr(), rtol, iters, stream=r.handle,
                             want_stats=want_stats, reads_back=want_stats or rtol > 0.0,
                             label="Pcg.solve %d iterations" % iters)
            r.snap(d_x)
            host.append((out if want_stats else None, cg.flavour()))
        return host
    return body


def _hp_check_cg(c, tag, b, x0, iters, got, rn, flavour, key, counts=None):
    """The default-stream result against hp.pcg, with compare's margin (test_gpu_cg.py)."""
    counts = counts or (iters,)
    ref = c.reference(b, x0, counts, key)
    tcg.compare(tag, c.n, flavour, iters, got, rn if rn is not None else float(ref[LD][1][iters]),
                ref[LD][0][iters], ref[LD][1][iters], ref[np.float64][0][iters], ref[np.float64][1][iters],
                check_resn=rn is not None)


@pytest.mark.parametrize("want_stats", [False, True])
@pytest.mark.parametrize("name", ["pair_small", "csr_small"])
def test_pcg_graph_replays_on_a_stream(schwz, oracle, torch_cuda, name, want_stats):
    """40 fixed iterations: two graph replays of 16 and eight loose iterations."""
    hp.require_extended_precision()
    shape, env = cc.GRIDS[name]
    mat = _lap(oracle, shape)
    c = tcg.grid_case(schwz, oracle, torch_cuda, name)
    b, x0 = cc.rhs(c.n, 1)
    (x,), host = rig.both(torch_cuda, _pcg_body(schwz, mat, env, [(b, x0, 0.0, 40, {})], want_stats),
                          "%s 40 iterations" % name)
    flavour = host[-1]
    assert flavour == c.expect(0.0, 40) and flavour & 4 == 0, flavour      # x in the loop: the graph plan
    if want_stats:
        assert host[0] == 40
    _hp_check_cg(c, "streams/%s/40" % name, b, x0, 40, x, host[1] if want_stats else None, flavour, "streams40")


@pytest.mark.parametrize("want_stats", [False, True])
@pytest.mark.parametrize("name", ["csr_small", "walk_small"])
def test_pcg_deferred_x_and_postponed_tail_on_a_stream(schwz, oracle, torch_cuda, name, want_stats):
    """SCHWZ_CG_DEFERX=2, 17 iterations: the ring of 16, the postponed tail (pcg_finish_lazy runs it inside the solve
    that asks for statistics; without them the second solve drops it), virtual first and last directions on the walk;
    then a second solve from another start vector on the same object and stream.  Pcg has no call that reads the
    statistics later: that route to pcg_finish_lazy (the tail launched afterwards, on the stream the solve remembered)
    is Subdomain.last_inner_stats, in test_ras_steps_on_a_stream[cg_deferx]."""
    hp.require_extended_precision()
    shape, env = cc.GRIDS[name]
    mat = _lap(oracle, shape)
    c = tcg.grid_case(schwz, oracle, torch_cuda, name)
    b, x0 = cc.rhs(c.n, 1)
    b2, x2 = cc.rhs(c.n, 77)
    solves = [(b, x0, 0.0, 17, D2), (b2, x2, 0.0, 6, D2)]
    (xa, xb), host = rig.both(torch_cuda, _pcg_body(schwz, mat, env, solves, want_stats), "%s deferred x" % name)
    fl = host[-1]
    assert fl == c.expect(0.0, 6, D2) and fl & 4, fl
    assert (fl & 128 == 128) == (name == "walk_small"), fl
    if want_stats:
        assert (host[0], host[3]) == (17, 6)
    _hp_check_cg(c, "streams/%s/lazy-first" % name, b, x0, 17, xa, host[1] if want_stats else None, fl, 0,
                 tcg.SMALL_COUNTS)
    _hp_check_cg(c, "streams/%s/lazy-second" % name, b2, x2, 6, xb, host[4] if want_stats else None, fl, "second")


@pytest.mark.parametrize("target", [17, 31])
@pytest.mark.parametrize("name,env_solve", [("pair_small", {}), ("walk_small", D2)])
def test_pcg_tolerance_stop_on_a_stream(schwz, oracle, torch_cuda, name, env_solve, target):
    """The polling path: two pinned banks and two events.  rtol from the longdouble history alone, separated from
    the reductions on either side by the margin Case.check_stop asserts -- on the CPU, before the device is asked."""
    hp.require_extended_precision()
    shape, env = cc.GRIDS[name]
    mat = _lap(oracle, shape)
    c = tcg.grid_case(schwz, oracle, torch_cuda, name)
    b, x0 = cc.rhs(c.n, 1)
    rtol = c.check_stop(b, x0, target, tcg.SMALL_COUNTS, env=env_solve)
    cap = max(4 * target, 64)
    for want_stats in (False, True):
        (x,), host = rig.both(torch_cuda, _pcg_body(schwz, mat, env, [(b, x0, rtol, cap, env_solve)], want_stats),
                              "%s stop at %d" % (name, target))
        if want_stats:
            assert host[0] == target
        _hp_check_cg(c, "streams/%s/stop%d" % (name, target), b, x0, target, x, host[1] if want_stats else None,
                     host[-1], 0, tcg.SMALL_COUNTS)


GENERAL = {"bj7": (2, 7, {}), "ilu": (3, 1, {}), "ilu_sweeps": (3, 1, dict(par_ilu_sweeps=3, trisolve_sweeps=2)),
           "isai": (4, 1, {})}


@pytest.mark.parametrize("pc", list(GENERAL))
def test_pcg_general_preconditioners_on_a_stream(schwz, oracle, torch_cuda, pc):
    """64 x 64 Laplacian: block-Jacobi 7, exact ILU(0) (the triangular solves inside the CG), ParILU factors applied
    by Jacobi sweeps, ISAI."""
    hp.require_extended_precision()
    precond, bs, kw = GENERAL[pc]
    rp, col, val = _lap(oracle, (64, 64))
    n = len(rp) - 1
    b, x0 = cc.rhs(n, 19)
    k = 6
    (x,), host = rig.both(torch_cuda, _pcg_body(schwz, (rp, col, val), {}, [(b, x0, 0.0, k, {})], True, precond, bs, **kw),
                          "general " + pc)
    (xn,), _ = rig.both(torch_cuda, _pcg_body(schwz, (rp, col, val), {}, [(b, x0, 0.0, k, {})], False, precond, bs, **kw),
                        "general %s, no statistics" % pc)
    assert rig.same(x, xn) and host[0] == k and host[-1] == 0
    if kw:
        f = schwz.parilu(rp, col, val, kw["par_ilu_sweeps"])
        L, U = hp.factors(f)
        M = {dt: (lambda v, dt=dt: hp.jacobi_sweep_solve(L, U, v, kw["trisolve_sweeps"], dtype=dt)) for dt in (LD, np.float64)}
    else:
        M = {dt: hp.make_precond(schwz, oracle, rp, col, val, precond, bs, dt) for dt in (LD, np.float64)}
    ref = {dt: hp.pcg(rp, col, val, b, x0, M[dt], k, dtype=dt) for dt in (LD, np.float64)}
    tcg.compare("streams/general/" + pc, n, 0, k, x, host[1], ref[LD][0], ref[LD][1][k], ref[np.float64][0],
                ref[np.float64][1][k])


def test_pcg_cached_graph_replayed_on_another_stream(schwz, oracle, torch_cuda):
    """The graph of (x, rtol) is recorded by a solve on the default stream; the same object then solves on S into the
    same x buffer (the cached graph is launched on another stream than the first time), and on S again."""
    hp.require_extended_precision()
    torch = torch_cuda
    name = "pair_small"
    shape, env = cc.GRIDS[name]
    mat = _lap(oracle, shape)
    c = tcg.grid_case(schwz, oracle, torch, name)
    b, x0 = cc.rhs(c.n, 1)

    def body(r):
        with cc.upload_env(env):
            A = r.hold(schwz.Csr(*mat))
            cg = r.hold(schwz.Pcg(A, 1))
        d_b0 = r.hold(torch.from_numpy(b).cuda())
        d_x = r.hold(torch.from_numpy(x0).cuda())
        cg.solve(d_b0.data_ptr(), d_x.data_ptr(), 0.0, 32, want_stats=False)       # records and caches the graph
        torch.cuda.synchronize()
        first = d_x.cpu().numpy()
        d_b = r.input(b)
        r.fill(d_x, x0)
        r.arm()
        r.call(cg.solve, d_b.data_ptr(), d_x.data_ptr(), 0.0, 32, stream=r.handle, want_stats=False)
        r.snap(d_x)
        r.call(cg.solve, d_b.data_ptr(), d_x.data_ptr(), 0.0, 32, stream=r.handle, want_stats=False)
        r.snap(d_x)
        return [first, cg.flavour()]
    (x1, x2), host = rig.both(torch, body, "cached graph")
    assert rig.same(host[0], x1) and not rig.same(x1, x2)
    assert host[1] == c.expect(0.0, 32)
    _hp_check_cg(c, "streams/cached-graph", b, x0, 32, x1, None, host[1], "streams32")


# ---- (c) the other solvers -----------------------------------------------------------------------------------------------

def _solver_body(make, b, x0, rtol, iters, want_stats, closed, stats_later=True):
    """make(r) -> the solver (held by the run).  want_stats=False: the statistics are read after the run has finished."""
    def body(r):
        s = make(r)
        d_b, d_x = r.input(b), r.input(x0)
        r.arm()
        out = r.call(s.solve, d_b.data_ptr(), d_x.data_ptr(), rtol, iters, stream=r.handle, want_stats=want_stats,
                     reads_back=not closed, label="%s.solve" % type(s).__name__)
        r.snap(d_x)
        if want_stats:
            return [out]
        return [s.last_stats] if stats_later and hasattr(s, "last_stats") else []
    return body


def _fixed_and_tolerance(torch, tag, make, b, x0, iters, rtol, cap):
    """One fixed-work and one tolerance solve, each with and without statistics.  Returns (x, its, resnorm) of the
    fixed-work reference run."""
    (x,), host = rig.both(torch, _solver_body(make, b, x0, 0.0, iters, True, False), tag + " fixed")
    (xn,), later = rig.both(torch, _solver_body(make, b, x0, 0.0, iters, False, True), tag + " fixed, no statistics")
    assert rig.same(x, xn), tag
    assert host[0] == iters
    if later:
        assert later[0] == iters and later[1] == host[1], (tag, later, host)
    (xt,), ht = rig.both(torch, _solver_body(make, b, x0, rtol, cap, True, False), tag + " tolerance")
    (xtn,), _ = rig.both(torch, _solver_body(make, b, x0, rtol, cap, False, False), tag + " tolerance, no statistics")
    assert rig.same(xt, xtn), tag
    assert 0 < ht[0] < cap, (tag, ht)         # it stopped on the tolerance: the host polled
    return x, host[0], host[1]


def _lap12(oracle):
    rp, col, val = oracle.laplacian3d(12, 12, 12)
    return np.asarray(rp, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64)


def test_pcg_f32_on_a_stream(schwz, oracle, torch_cuda):
    hp.require_extended_precision()
    name, k = "lap3d_12x12x12", 10
    rp, col, val = tgm._matrix(name)
    b, x0 = tgm._problem(name)

    def make(r):
        return r.hold(schwz.PcgF32(r.hold(schwz.Csr(rp, col, val)), 1))
    x, _, rn = _fixed_and_tolerance(torch_cuda, "PcgF32", make, b, x0, k, 1e-4, 400)
    ref = tgm._fixed_reference(name, 1)
    x_ld, x_32 = ref[LD][k], ref[np.float32][k]
    delta = float(np.linalg.norm((x_32 - x_ld).astype(np.float64)))
    err = float(np.linalg.norm((x.astype(LD) - x_ld).astype(np.float64)))
    assert np.isfinite(rn) and err <= 8 * delta, (err, delta)


@pytest.mark.parametrize("pc", [0, 1])
def test_chebyshev_on_a_stream(schwz, oracle, torch_cuda, pc):
    """Also with h_resnorm requested after a fixed-work solve: one more matrix pass, which must store nothing (the x of
    the run with statistics is the x of the run without)."""
    hp.require_extended_precision()
    rp, col, val = _lap12(oracle)
    n = len(rp) - 1
    b, x0 = cc.rhs(n, 29)
    lmin, lmax = (0.025, 2.0) if pc else (0.15, 12.0)
    k = 11

    def make(r):
        s = r.hold(schwz.Chebyshev(r.hold(schwz.Csr(rp, col, val)), pc))
        s.set_bounds(lmin, lmax)
        return s
    x, _, rn = _fixed_and_tolerance(torch_cuda, "Chebyshev pc %d" % pc, make, b, x0, k, 1e-3, 400)
    diag = hp_chebyshev.diagonal(rp, col, val) if pc else None
    ref = {dt: hp_chebyshev.chebyshev(rp, col, val, b, x0, diag, lmin, lmax, k, dtype=dt) for dt in (LD, np.float64)}
    tcg.compare("streams/chebyshev/%d" % pc, n, 0, k, x, rn, ref[LD][0], ref[LD][1][k], ref[np.float64][0],
                ref[np.float64][1][k])


@pytest.mark.parametrize("restart,k", [(4, 7), (30, 23)])
def test_gmres_on_a_stream(schwz, oracle, torch_cuda, convdiff, restart, k):
    """GMRES looks at its state one cycle behind the launches, whatever rtol is: the fixed-work solves here have at most
    two cycles (BiCGSTAB: fewer than two polling batches), so that they return without having waited."""
    hp.require_extended_precision()
    rp, col, val = convdiff(40)
    n = len(rp) - 1
    b, x0 = cc.rhs(n, 29)

    def make(r):
        return r.hold(schwz.Gmres(r.hold(schwz.Csr(rp, col, val)), 1, 1, restart))
    x, _, rn = _fixed_and_tolerance(torch_cuda, "Gmres(%d)" % restart, make, b, x0, k, 1e-2, 2000)
    M = {dt: hp.make_precond(schwz, oracle, rp, col, val, 1, 1, dt) for dt in (LD, np.float64)}
    ref = {dt: hp.gmres(rp, col, val, b, x0, M[dt], k, restart, 0.0, dt) for dt in (LD, np.float64)}
    tcg.compare("streams/gmres/%d" % restart, n, 0, k, x, rn, ref[LD][0], ref[LD][1][-1], ref[np.float64][0],
                ref[np.float64][1][-1])


def test_bicgstab_on_a_stream(schwz, oracle, torch_cuda, convdiff):
    hp.require_extended_precision()
    rp, col, val = convdiff(40)
    n = len(rp) - 1
    b, x0 = cc.rhs(n, 29)
    k = 11

    def make(r):
        return r.hold(schwz.Bicgstab(r.hold(schwz.Csr(rp, col, val)), 1))
    x, _, rn = _fixed_and_tolerance(torch_cuda, "Bicgstab", make, b, x0, k, 1e-6, 2000)
    M = {dt: hp.make_precond(schwz, oracle, rp, col, val, 1, 1, dt) for dt in (LD, np.float64)}
    ref = {dt: hp_bicgstab.bicgstab(rp, col, val, b, x0, M[dt], k, 0.0, dt) for dt in (LD, np.float64)}
    assert len(ref[LD][1]) - 1 == k and ref[LD][3] == 0
    tcg.compare("streams/bicgstab", n, 0, k, x, rn, ref[LD][0], ref[LD][1][k], ref[np.float64][0], ref[np.float64][1][k])


# ---- (d) Trs -------------------------------------------------------------------------------------------------------------

def _trs_factors(kind):
    rng = np.random.default_rng(len(kind) + 40)
    if kind == "one_workgroup":          # n <= 8192 with a permutation
        n = 65
        f = hp.five_point_factors(n, 8, rng)
        p = rng.permutation(n).astype(np.int32)
        return f, (p, p), {}
    if kind == "flags":                  # n = 8193 without one: the lane-per-row flag sweep
        return hp.five_point_factors(8193, 90, rng), None, {}
    if kind == "flag_wave":              # LU factors with rows of several waves
        n = 8300
        f = hp.banded_factors(n, 200, 300, rng)
        assert np.diff(f["l_rp"]).max() > 64
        return f, (rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)), {}
    if kind == "level_plan":             # 24 segments per factor: captured into a graph per (b, y)
        return hp.layered_factors(ttrs.WIDTHS, rng), None, {"SCHWZ_TRS_FLAGS": "0"}
    assert kind == "sweeps"
    return hp.five_point_factors(5000, 70, rng), "sweeps", {}


@pytest.mark.parametrize("kind", ["one_workgroup", "flags", "flag_wave", "level_plan", "sweeps"])
def test_trs_on_a_stream(schwz, torch_cuda, kind):
    """Each object solves twice on S with the same (b, y), then once with another pair: on the level plan the first
    call captures, the second replays the cached graph, the third captures again."""
    hp.require_extended_precision()
    f, perms, env = _trs_factors(kind)
    n = len(f["l_rp"]) - 1
    rng = np.random.default_rng(n)
    b1, b2 = rng.standard_normal(n), rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-8, 9, n))
    args = (f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"])

    def body(r):
        with cc.upload_env(env):
            t = r.hold(schwz.TrsSweeps(*args, 3) if perms == "sweeps" else ttrs._make(schwz, f, perms))
        d_b1, d_b2, d_y1, d_y2 = r.input(b1), r.input(b2), r.output(n), r.output(n)
        r.arm()
        for d_b, d_y in ((d_b1, d_y1), (d_b1, d_y1), (d_b2, d_y2)):
            r.call(t.solve, d_b.data_ptr(), d_y.data_ptr(), stream=r.handle, label="Trs.solve " + kind)
            r.snap(d_y)
    (y1, y1b, y2), _ = rig.both(torch_cuda, body, "trs " + kind)
    assert rig.same(y1, y1b)
    if perms == "sweeps":
        L, U = hp.factors(f)
        for b, y in ((b1, y1), (b2, y2)):
            y_ref, bound = hp.jacobi_sweep_solve(L, U, b, 3, bound=True)
            assert np.isfinite(y).all() and (np.abs(y.astype(LD) - y_ref) <= 2 * bound).all()
    else:
        ref = ttrs.Reference(f, perms)
        ref.check(b1, y1, "streams/trs %s rhs 1" % kind)
        ref.check(b2, y2, "streams/trs %s rhs 2" % kind)


# ---- (e) one RAS step sequence ---------------------------------------------------------------------------------------------

# local solver -> (partition, options of to_device, setter after it, switches in force)
LOCAL = {
    "cg": ("band_p3", {}, None, {}),
    "cg_deferx": ("band_p3", {}, None, D2),      # the deferred x and the postponed tail, read through last_inner_stats
    "direct_llt": ("band_p3", dict(local_solver=1), None, {}),
    "direct_lu": ("band_p3", dict(local_solver=2), None, {}),
    "gmres": ("nonsym_band_p3", dict(non_symmetric=True, restart_iter=4), None, {}),
    "bicgstab": ("nonsym_band_p3", dict(non_symmetric=True, restart_iter=4),
                 lambda sd, capi: sd.set_nonsym_solver(capi.NONSYM_BICGSTAB), {}),
    "chebyshev": ("band_p3", {}, lambda sd, capi: sd.set_sym_solver(capi.SYM_CHEBYSHEV), {}),
    "f32": ("band_p3", {}, lambda sd, capi: sd.set_local_precision(capi.PRECISION_F32), {}),
}
INNER = 7


def _ras_body(schwz, torch, kind):
    name, kw, setter, env = LOCAL[kind]

    def body(r):
        with cc.upload_env(env):
            return steps_on(r)

    def steps_on(r):
        R = r.hold(steps.StepRig(schwz, torch, name, {}, maxit=INNER, device_kw=kw))
        sds = R.sds
        send, recv, send32, recv32, early, normsq, true_x = {}, {}, {}, {}, {}, {}, {}
        for me, sd in sds.items():
            if setter:
                setter(sd, schwz.capi)
            send[me], recv[me] = r.output(sd.num_send), r.output(sd.num_recv)
            send32[me] = r.output(sd.num_send, np.float32)
            recv32[me] = r.input(np.random.default_rng(90 + me).standard_normal(sd.num_recv).astype(np.float32))
            early[me], normsq[me] = r.output(sd.num_send), r.output(1)
            true_x[me] = r.hold(torch.from_numpy(R.x[me]).cuda())
            # y starts as x~ on the local rows, as it stands between a restriction and the next solve (the fused check
            # launch relies on it: test_gpu_ras_steps.py); in the gated run both are poison until the gate has passed
            n = sd.local_size_x
            R.put(me, 2, np.full(n, np.nan) if r.gated else R.x[me][:n])
            if r.gated:
                R.put(me, 0, np.full(len(R.x[me]), np.nan))
        # host-side index work, done before the gate: offsets, who sends what to whom, whether the solver packs early
        soff = {me: sd.send_offsets() for me, sd in sds.items()}
        roff = {me: sd.recv_offsets() for me, sd in sds.items()}
        puts = {me: [q for q, _ in sd.put_lists()] for me, sd in sds.items()}
        src = {me: [(p, puts[p].index(me)) for p, _ in sd.get_lists()] for me, sd in sds.items()}
        epk = {me: bool(sd.early_pack_ok()) for me, sd in sds.items()}
        side = r.hold(rig.stream_beside_default(torch)) if r.gated else None      # the second, non-blocking stream
        side_handle = side.cuda_stream if r.gated else 0
        r.arm()
        if r.gated:                                       # behind the gate's event: x~ takes its true values
            for me, sd in sds.items():
                for which in (0, 2):
                    p, cnt = sd.vector(which)
                    schwz.gather(cnt, R.idx[me].data_ptr(), true_x[me].data_ptr(), p, stream=r.handle)

        def snap_state(me):
            for which in (0, 1, 2):                       # x~, b~, y
                p, cnt = sds[me].vector(which)
                t = r.output(cnt)
                schwz.gather(cnt, R.idx[me].data_ptr(), p, t.data_ptr(), stream=r.handle)
                r.snap(t)
        host, early_at, pend = [], [], []
        t0 = time.perf_counter()
        for outer in range(2):
            # The first outer iteration is enqueued whole -- every subdomain, the restriction and the one-off forms
            # included -- before anything reads back: the gate is shut at the return of every one of these calls.  (A
            # host may restrict before it has read the norm: the restriction does not touch the scalar.)  The second
            # one runs after the read-backs of the first, on an open gate: its values are compared, no more.
            late = not (outer == 0)
            for me, sd in sds.items():
                r.call(sd.pack, send[me].data_ptr(), stream=r.handle, reads_back=late)
                r.snap(send[me])
            for me, sd in sds.items():
                with r.on_stream():                       # the exchange: torch copies on the run's stream
                    for k, (p, j) in enumerate(src[me]):
                        recv[me][roff[me][k]:roff[me][k + 1]].copy_(send[p][soff[p][j]:soff[p][j + 1]])
                r.call(sd.unpack, recv[me].data_ptr(), stream=r.handle, reads_back=late)
                r.call(sd.update_boundary, stream=r.handle, reads_back=late)
                r.call(sd.check_and_solve_launch, stream=r.handle, reads_back=late)
                if epk[me]:
                    r.call(sd.pack_early, early[me].data_ptr(), stream=side_handle, reads_back=late)
                r.call(sd.norm_sq_to_device, normsq[me].data_ptr(), stream=side_handle, reads_back=late)
                r.call(sd.restrict, stream=r.handle, reads_back=late)
                snap_state(me)
                if epk[me]:
                    after = r.output(sd.num_send)
                    r.call(sd.pack, after.data_ptr(), stream=r.handle, reads_back=late)
                    pend.append((me, len(r.snaps)))
                    r.snap(after)                         # (early[me] is snapped once the second stream is done)
            if outer == 0:                                # the fp32 and the per-neighbour forms, once each
                for me, sd in sds.items():
                    r.call(sd.pack_f32, send32[me].data_ptr(), stream=r.handle)
                    r.snap(send32[me])
                    for k in range(sd.num_neighbors_out):
                        one = r.output(soff[me][k + 1] - soff[me][k])
                        one32 = r.output(soff[me][k + 1] - soff[me][k], np.float32)
                        r.call(sd.pack_neighbor, k, one.data_ptr(), single=False, stream=r.handle)
                        r.call(sd.pack_neighbor, k, one32.data_ptr(), single=True, stream=r.handle)
                        r.snap(one)
                        r.snap(one32)
                    r.call(sd.unpack_f32, recv32[me].data_ptr(), stream=r.handle)
                    snap_state(me)
                    for k in range(sd.num_neighbors_in):
                        r.call(sd.unpack_neighbor, k, recv[me].data_ptr() + 8 * roff[me][k], single=False, stream=r.handle)
                    snap_state(me)
                    for k in range(sd.num_neighbors_in - 1, -1, -1):
                        r.call(sd.unpack_neighbor, k, recv32[me].data_ptr() + 4 * roff[me][k], single=True, stream=r.handle)
                    snap_state(me)
                r.check_shut("the first outer iteration of %s, enqueued whole" % kind)
                if not r.gated:
                    rig.CALL_LOG.append(("the first outer RAS iteration (%s), all its calls together" % kind,
                                         (time.perf_counter() - t0) * 1e3))
            # ---- the read-backs of this outer iteration
            for me, sd in sds.items():
                if kind.startswith("cg"):
                    # the statistics nobody asked the solve for: the postponed launches of a deferred-x solve run now,
                    # on the stream the solve remembered -- for subdomain 0 of the first iteration behind a shut gate
                    assert (sd.cg_flavour() & 4 == 4) == (kind == "cg_deferx"), sd.cg_flavour()
                    its, rn = r.call(sd.last_inner_stats, reads_back=True)
                    assert its == INNER
                    host.append(rn)
                    snap_state(me)
                lres = r.call(sd.local_residual_wait, reads_back=True)
                if r.gated:
                    side.synchronize()
                else:
                    torch.cuda.synchronize()
                sq = float(normsq[me].cpu().numpy()[0])
                # local_residual_wait returns the root of the squared norm the device holds: the same scalar
                assert np.sqrt(sq) == lres, (kind, me, sq, lres)
                host.append(lres)
            for me, k in pend:                            # (the second stream is done: synchronised above)
                early_at.append((k, len(r.snaps)))
                r.snap(early[me])
            pend.clear()
        for me, sd in sds.items():
            host.append(sd.true_residual_sq(stream=r.handle))
            host.append(sd.get_interior(stream=r.handle))
        return [host, [np.array(early_at, dtype=np.int64).reshape(-1, 2)]]
    return body


@pytest.mark.parametrize("kind", list(LOCAL))
def test_ras_steps_on_a_stream(schwz, torch_cuda, kind):
    """band_p3 (three subdomains, overlap 2), two outer iterations of pack -> exchange -> unpack -> update_boundary ->
    check_and_solve_launch -> restrict on S, the early pack and the norm for the device-side all-gather on a second
    non-blocking stream, and once each pack_f32 / unpack_f32 / pack_neighbor / unpack_neighbor in both widths; then
    last_inner_stats (CG), local_residual_wait, and at the end true_residual_sq and get_interior.  x~, b~ and y against
    the default-stream run after every step.  The first outer iteration of all three subdomains is enqueued behind the
    shut gate, every call asserted to return before it opens; the second runs on an open gate (values only)."""
    torch = torch_cuda
    snaps, host = rig.both(torch, _ras_body(schwz, torch, kind), "ras steps " + kind)
    early_at = host[-1]
    if kind != "cg_deferx":
        assert (len(early_at) > 0) == (kind == "cg")
    for a, b in early_at:
        assert rig.same(snaps[a], snaps[b]) and np.abs(snaps[a]).max() > 0         # pack after restrict == pack_early
    assert np.isfinite(host[0]) and host[0] > 0


def test_ras_step_norms_of_the_default_stream_run_meet_their_bounds(schwz, torch_cuda):
    """The reference side of (e), once: the check norm of the first step against hp.residual / hp.norm_sq_bound."""
    hp.require_extended_precision()
    torch = torch_cuda
    R = steps.StepRig(schwz, torch, "band_p3", {}, maxit=INNER)
    R.exchange_and_update()
    for me, sd in R.sds.items():
        n = sd.local_size_x
        rp, col, val = sd.local_matrix()
        x, bt = R.get(me, 0)[:n], R.get(me, 1)
        R.put(me, 2, x)                                   # y is x~ on the local rows, as in the step sequence
        r_ = hp.residual(rp, col, val, x, bt)
        e = hp.residual_bound(rp, col, val, x, bt)
        B = hp.norm_sq_bound(r_, e, n, root=True)
        sd.check_and_solve_launch()
        got = sd.local_residual_wait()
        torch.cuda.synchronize()
        assert abs(hp.LD(got) ** 2 - np.sum(r_ * r_)) <= B, (me, got)


# ---- (f) the Python host ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["synchronous", "overlapped"])
def test_python_host_with_a_non_default_current_stream(schwz, torch_cuda, mode):
    """SolverRAS inside `with torch.cuda.stream(S)`: backend.stream() hands S to every call.  Ungated: nothing may
    break or differ when the current stream is not the default stream."""
    torch = torch_cuda

    def run(stream):
        s = schwz.Settings()
        if mode == "overlapped":
            s.comm_settings.enable_onesided = True
            s.comm_settings.enable_overlap = True
            s.convergence_settings.enable_decentralized_leader_election = True
        m = schwz.Metadata(num_subdomains=3, oned_laplacian_size=32, tolerance=1e-6, max_iters=600)
        solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(3), quiet=True)
        if stream is None:
            solver.initialize()
            out = solver.run()
        else:
            with torch.cuda.stream(stream):
                solver.initialize()
                out = solver.run()
        ppd = m.post_process_data      # the synchronous loop records the global norms, the overlapped one the local ones
        hist = [np.asarray(h, dtype=np.float64) for h in ppd["global_residual_vector_out"]]
        hist.append(np.asarray(ppd["local_residual_vector_out"], dtype=np.float64))
        return out, hist
    ref, hist_ref = run(None)
    got, hist = run(torch.cuda.Stream())
    assert ref["converged"] and got["converged"]
    assert got["iter_count"] == ref["iter_count"]
    assert rig.same(got["solution"], ref["solution"])
    assert len(hist) == len(hist_ref) and all(rig.same(a, b) for a, b in zip(hist, hist_ref))
    assert sum(len(h) for h in hist_ref) > 0


# ---- (g) creation is complete on return ------------------------------------------------------------------------------------

def _after_creation(torch, prepare, make_and_use):
    """prepare() -> device buffers; make_and_use(buffers, stream handle, stream context) -> result tensors (and whatever
    must outlive the use).  Once plainly on the default stream; once with the delay queued on the DEFAULT stream before
    the creation calls and the object used on S at once, with no gate and no synchronisation of the test's own in
    between.  A creation call that left work pending would have it run after the use.

    How much this can show (read from the code, not measured): every creation path begins with blocking default-stream
    uploads (hipMemcpy), which wait for the delay, so the delay is over when the first of them returns; asynchronous
    work at the END of a create is then exposed only for the microseconds until the first launch on S.  The cases
    follow the recipe and would catch a create that returns with a long queue behind it; that they pass is weak
    evidence for a trailing memset."""
    bufs = prepare()
    torch.cuda.synchronize()
    held_ref = make_and_use(bufs, 0, rig._Null())
    torch.cuda.synchronize()
    ref = [t.cpu().numpy() for t in held_ref[0]]
    bufs = prepare()
    S = rig.stream_beside_default(torch)
    torch.cuda.synchronize()
    rig.delay(torch)                                     # on the default stream
    held = make_and_use(bufs, S.cuda_stream, torch.cuda.stream(S))
    S.synchronize()
    got = [t.cpu().numpy() for t in held[0]]
    torch.cuda.synchronize()
    assert len(ref) == len(got)
    for k, (a, b) in enumerate(zip(ref, got)):
        assert rig.same(a, b), "result %d differs when the object is used right after its creation" % k
    return got


@pytest.mark.parametrize("solver", ["Pcg", "PcgF32", "Chebyshev", "Gmres", "Bicgstab"])
def test_solver_creation_is_complete_on_return(schwz, oracle, torch_cuda, convdiff, solver):
    """Csr and the solver are created behind a busy default stream and solve five iterations on S at once."""
    torch = torch_cuda
    rp, col, val = convdiff(40) if solver in ("Gmres", "Bicgstab") else _lap12(oracle)
    n = len(rp) - 1
    b, x0 = cc.rhs(n, 3)
    make = {"Pcg": lambda A: schwz.Pcg(A, 1), "PcgF32": lambda A: schwz.PcgF32(A, 1),
            "Chebyshev": lambda A: schwz.Chebyshev(A, 1), "Gmres": lambda A: schwz.Gmres(A, 1, 1, 4),
            "Bicgstab": lambda A: schwz.Bicgstab(A, 1)}[solver]

    def prepare():
        return torch.from_numpy(b).cuda(), torch.from_numpy(x0).cuda()

    def make_and_use(bufs, handle, on):
        d_b, d_x = bufs
        A = schwz.Csr(rp, col, val)
        s = make(A)
        s.solve(d_b.data_ptr(), d_x.data_ptr(), 0.0, 5, stream=handle, want_stats=False)
        with on:
            out = d_x.clone()
        return [out], A, s
    x, = _after_creation(torch, prepare, make_and_use)
    assert np.isfinite(x).all() and not np.array_equal(x, x0)


def test_trs_creation_is_complete_on_return(schwz, torch_cuda):
    torch = torch_cuda
    f, perms, _ = _trs_factors("flags")
    n = len(f["l_rp"]) - 1
    b = np.random.default_rng(5).standard_normal(n)

    def prepare():
        return torch.from_numpy(b).cuda(), torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")

    def make_and_use(bufs, handle, on):
        d_b, d_y = bufs
        t = ttrs._make(schwz, f, perms)
        t.solve(d_b.data_ptr(), d_y.data_ptr(), stream=handle)
        with on:
            out = d_y.clone()
        return [out], t
    y, = _after_creation(torch, prepare, make_and_use)
    assert np.isfinite(y).all()


def test_subdomain_upload_and_window_are_zero_on_return(schwz, torch_cuda):
    """Subdomain.to_device: local_residual on S must see x~ = 0, so the norm is |rhs|; DeviceWindow: reads back zeros."""
    torch = torch_cuda
    rp, col, val, P, _, _ = steps.global_case("band_p3")
    prob = schwz.Problem.from_csr(rp, col, val)
    fr = schwz.partition_regular(prob.N, P)
    count = 4096
    norms = []

    def prepare():
        return (torch.arange(count, dtype=torch.int32, device="cuda"),
                torch.full((count,), float("nan"), dtype=torch.float64, device="cuda"))

    def make_and_use(bufs, handle, on):
        idx, dst = bufs
        sd = schwz.Subdomain(prob, P, 1, 2, fr)
        rhs = np.random.default_rng(8).standard_normal(sd.local_size_x)
        sd.to_device(rhs, precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=3)
        lres = sd.local_residual(stream=handle)
        w = schwz.DeviceWindow(count)
        schwz.gather(count, idx.data_ptr(), w.ptr, dst.data_ptr(), stream=handle)
        with on:
            out = dst.clone()
        norms.append((lres, float(np.sqrt(np.sum(rhs.astype(LD) ** 2)))))
        return [out], sd, w
    z, = _after_creation(torch, prepare, make_and_use)
    assert not z.any()
    assert norms[0][0] == norms[1][0]
    assert abs(norms[1][0] - norms[1][1]) <= 1e-13 * norms[1][1], norms      # |rhs| of some 500 entries: x~ was zero


# ---- (h) independent objects on several streams at once ----------------------------------------------------------------------

def _concurrently(torch, bodies, tag):
    """bodies: (setup(run) -> launch(run)) per stream.  Each alone on the default stream first (the reference), then
    all of them gated on streams of their own at once.  Up to three streams are probed to run beside each other
    (rig.streams_beside_each_other): their work overlaps on the device.  With more streams than the process has
    hardware queues some of them share one and serialise; they are still distinct streams, each beside the default
    stream."""
    refs = []
    for setup in bodies:
        r = rig.Run(torch, False)
        launch = setup(r)
        r.arm()
        launch(r)
        refs.append(r.finish())
        del r, launch
    if len(bodies) <= 3:
        runs = [rig.Run(torch, True, stream=S) for S in rig.streams_beside_each_other(torch, len(bodies))]
    else:
        runs = [rig.Run(torch, True) for _ in bodies]
    assert len({r.handle for r in runs}) == len(runs), "%s: the streams are not distinct" % tag
    launches = [setup(r) for setup, r in zip(bodies, runs)]
    for k, r in enumerate(runs):
        r.arm(sync=(k == 0))
    for launch, r in zip(launches, runs):
        launch(r)
    for r in runs:
        r.check_shut(tag + ": all solves enqueued")
    for k, (r, ref) in enumerate(zip(runs, refs)):
        rig.assert_same((ref, []), (r.finish(), []), "%s: stream %d" % (tag, k))


def _solve_setup(make, b, x0, iters):
    def setup(r):
        s = make(r)
        d_b, d_x = r.input(b), r.input(x0)

        def launch(r):
            r.call(s.solve, d_b.data_ptr(), d_x.data_ptr(), 0.0, iters, stream=r.handle, want_stats=False)
            r.snap(d_x)
        return launch
    return setup


def test_two_pcg_on_two_matrices_on_two_streams(schwz, oracle, torch_cuda):
    bodies = []
    for name, seed in (("pair_small", 1), ("csr_small", 2)):
        shape, env = cc.GRIDS[name]
        mat = _lap(oracle, shape)
        b, x0 = cc.rhs(len(mat[0]) - 1, seed)

        def make(r, mat=mat, env=env):
            with cc.upload_env(env):
                return r.hold(schwz.Pcg(r.hold(schwz.Csr(*mat)), 1))
        bodies.append(_solve_setup(make, b, x0, 20))
    _concurrently(torch_cuda, bodies, "two Pcg, two matrices")


def test_four_solvers_on_one_matrix_on_four_streams(schwz, oracle, torch_cuda):
    """Pcg, Chebyshev, PcgF32 and Gmres created on ONE Csr, as a subdomain creates them."""
    rp, col, val = _lap12(oracle)
    n = len(rp) - 1
    shared = {}

    def matrix(r):
        # one matrix per pass: the reference runs share one, the concurrent runs share another
        key = r.gated
        if key not in shared:
            shared[key] = schwz.Csr(rp, col, val)
        return shared[key]
    kinds = [lambda A: schwz.Pcg(A, 1), lambda A: schwz.Chebyshev(A, 1), lambda A: schwz.PcgF32(A, 1),
             lambda A: schwz.Gmres(A, 1, 1, 4)]
    bodies = []
    for k, kind in enumerate(kinds):
        b, x0 = cc.rhs(n, 50 + k)
        bodies.append(_solve_setup(lambda r, kind=kind: r.hold(kind(matrix(r))), b, x0, 7))
    _concurrently(torch_cuda, bodies, "four solvers, one matrix")
    torch_cuda.cuda.synchronize()
    shared.clear()


STREAM_TILES = 8200      # tiles of 256 rows: more than 4 * kMaxGrid = 8192, where the stream kernel folds through scratch


def _tridiagonal(n):
    """Tridiagonal SPD matrix with random couplings in (-1, 0) and a diagonal in (3, 4)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(n % 9973)
    off, dg = rng.uniform(-1, 0, n - 1), rng.uniform(3, 4, n)
    a = sp.diags([off, dg, off], [-1, 0, 1], shape=(n, n), format="csr")
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def test_two_pcg_on_one_plain_matrix_on_two_streams(schwz, torch_cuda):
    """Two Pcg on ONE plain-CSR matrix of 8200 x 256 rows (three entries per row, 75 MB), six iterations each on two
    streams at once.  Past 4 * 2048 tiles the stream kernel's short-lived workgroups fold their partial sums through
    scratch; that scratch belongs to the object that launches, not to the matrix, so the two solves do not meet.
    Rows of at most three entries: every tile has 256 rows (tile rule of schwz_csr_create, hp.tiles_of), 8200 tiles.
    The two streams are probed to run beside each other, so the solves overlap.  Pcg exposes nothing that tells whether
    a launch took the folded form (a failed scratch allocation quietly keeps the persistent grid, as it did when the
    matrix owned the scratch): plain coding, the row count and flavour 4 are what can be asserted here; that the case
    discriminates is on record for the matrix-owned scratch (profiles/r17_stream_contract.txt)."""
    n = STREAM_TILES * 256
    rp, col, val = _tridiagonal(n)
    assert np.diff(rp).max() * hp.TILE_ROWS <= hp.TILE_NNZ - 2 and -(-n // hp.TILE_ROWS) > 4 * 2048
    assert list(hp.tiles_of(rp[:256 * 5 + 1])) == [0, 256, 512, 768, 1024, 1280]
    with cc.upload_env(cc.PLAIN):
        A = schwz.Csr(rp, col, val)
    # plain coding and the row count: what sends this matrix's products to the stream kernel's folded form
    assert A.format() == 0 and A.nrows == n and n > cc.GRAPH_ROWS
    solvers = []
    bodies = []
    for k in range(2):
        b, x0 = cc.rhs(n, 60 + k)

        def make(r):
            solvers.append(schwz.Pcg(A, 1))
            return r.hold(solvers[-1])
        bodies.append(_solve_setup(make, b, x0, 6))
    _concurrently(torch_cuda, bodies, "two Pcg, one plain matrix")
    assert all(s.flavour() == 4 for s in solvers)      # stored q, deferred x: the stream kernel carries p.(A p)
    torch_cuda.cuda.synchronize()
    solvers.clear()


# ---- the rig can fail ----------------------------------------------------------------------------------------------------------

def test_rig_detects_a_launch_on_the_wrong_stream(schwz, torch_cuda, monkeypatch):
    """core._stream_arg patched to hand every call the default stream: the gather runs while the gate is shut, reads
    the NaN poison, and the comparison must fail.  (Nothing is provoked: the kernel reads valid memory that holds NaN;
    INDEX_POISON is a valid index.)  That it fails is also what shows S to be non-blocking."""
    n = 1000
    m, idx, frm_g, into_g, frm_s, into_s = _gather_scatter_inputs(n)
    body = _gather_scatter_body(schwz, n, m, idx, frm_g, into_g, frm_s, into_s, schwz.capi.OP_COPY)
    rig.both(torch_cuda, body, "control, unpatched")
    monkeypatch.setattr(schwz.core, "_stream_arg", lambda stream: None)
    with pytest.raises(AssertionError, match="differs from the default-stream run"):
        rig.both(torch_cuda, body, "control")
    torch_cuda.cuda.synchronize()


def test_rig_detects_a_solve_on_the_wrong_stream(schwz, oracle, torch_cuda, monkeypatch):
    """The same for a Pcg solve: b is still NaN when the misdirected solve runs."""
    shape, env = cc.GRIDS["pair_small"]
    mat = _lap(oracle, shape)
    b, x0 = cc.rhs(len(mat[0]) - 1, 1)
    body = _pcg_body(schwz, mat, env, [(b, x0, 0.0, 5, {})], False)
    rig.both(torch_cuda, body, "control, unpatched")
    monkeypatch.setattr(schwz.core, "_stream_arg", lambda stream: None)
    with pytest.raises(AssertionError, match="differs from the default-stream run"):
        rig.both(torch_cuda, body, "control")
    torch_cuda.cuda.synchronize()
