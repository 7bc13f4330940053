"""The fixed part of a local CG solve: where its result is stored and who initialises CgState.

1. On a subdomain without overlap and halo whose CG defers the x update, y lives in one of the two x~ buffers
   (schwz_ras_y_form 1 / 2) and the last x update stores the solution once.  SCHWZ_RESTRICT_FUSE=0 keeps y in a
   buffer of its own.  No arithmetic differs, so every vector and every norm of the two forms must be equal bit for
   bit -- step by step, and through the odd sequences of calls (a solve that is not restricted, a restriction without
   a solve, a write into y, a switch of form between two solves).
2. Where a solve starts in the z-sweep walk, workgroup 0 of the first-direction launch folds the start launch's
   partial sums into CgState and the check norm (SCHWZ_CG_INITFOLD=0: cg_init_finalize_kernel on its own).  The same
   folds in the same order: equal bits again.

One recorded script per subdomain and set of switches: every operation of the script leaves what it returned and
y and x~[:n] in the record, and the tests compare records.  The vectors are kept as digests of their bytes (a run
over 128 x 128 x 129 would otherwise hold gigabytes): for finite vectors with -0.0 folded into 0.0, which is what
is digested, equal digests are numpy.array_equal."""
import hashlib

import numpy as np
import pytest

import cg_child as cc

pytestmark = pytest.mark.gpu

PAST128 = cc.GRIDS["past128"][0]     # 128 x 128 x 129: the smallest grid with flavour 254 without switches
SMALL = (5, 7, 9)                    # 315 rows: odd n, no walk, x deferred only by SCHWZ_CG_DEFERX=2
SLABS = (128, 128, 144)              # three z-slabs of 128 x 128 x 48
K = 10

FUSE0 = {"SCHWZ_RESTRICT_FUSE": "0"}
FOLD0 = {"SCHWZ_CG_INITFOLD": "0"}


class Rig:
    """P subdomains of one grid on the device, driven op by op; P > 1 exchanges halos through torch buffers."""

    def __init__(self, schwz, torch, shape, P, env, seed=1, **dev):
        self.schwz, self.torch, self.P = schwz, torch, P
        prob = schwz.Problem.laplacian(3, *shape)
        fr = schwz.partition_regular(prob.N, P)
        self.sds = [schwz.Subdomain(prob, P, me, 2, fr) for me in range(P)]
        if P > 1:
            lists = schwz.InProcessComm(P).handshake({me: sd.get_lists() for me, sd in enumerate(self.sds)})
            for me, lst in lists.items():
                for q, ids in lst:
                    self.sds[me].add_put_list(q, ids)
        self.env = dict(env)
        self.b, self.send, self.recv, self.idx = [], [], [], []
        with cc.upload_env(self.env):
            for sd in self.sds:
                b, _ = cc.rhs(sd.local_size_x, seed)
                self.b.append(b)
                sd.to_device(b, precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=K, **dev)
                self.send.append(torch.zeros(max(sd.num_send, 1), dtype=torch.float64, device="cuda"))
                self.recv.append(torch.zeros(max(sd.num_recv, 1), dtype=torch.float64, device="cuda"))
                self.idx.append(torch.arange(sd.local_size_x, dtype=torch.int32, device="cuda"))
        self.forms = []   # schwz_ras_y_form of every subdomain after every op
        self.flavours = []
        self.flavours_after = []   # schwz_ras_cg_flavour of every subdomain after every op

    def get(self, me, which):
        sd, torch = self.sds[me], self.torch
        n = sd.local_size_x
        p, cnt = sd.vector(which)
        assert cnt >= n
        t = torch.empty(n, dtype=torch.float64, device="cuda")
        self.schwz.gather(n, self.idx[me].data_ptr(), p, t.data_ptr())
        torch.cuda.synchronize()
        return t.cpu().numpy()

    def put(self, me, which, a):
        sd, torch = self.sds[me], self.torch
        n = sd.local_size_x
        p, _ = sd.vector(which)
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        self.schwz.gather(n, self.idx[me].data_ptr(), t.data_ptr(), p)
        torch.cuda.synchronize()

    def exchange(self):
        if self.P == 1:
            return
        bufs = {}
        for me, sd in enumerate(self.sds):
            sd.pack(self.send[me].data_ptr())
            off = sd.send_offsets()
            for k, (q, _) in enumerate(sd.put_lists()):
                bufs[(me, q)] = self.send[me][off[k]:off[k + 1]]
        self.torch.cuda.synchronize()
        for me, sd in enumerate(self.sds):
            off = sd.recv_offsets()
            for k, (p, _) in enumerate(sd.get_lists()):
                self.recv[me][off[k]:off[k + 1]].copy_(bufs[(p, me)])
            sd.unpack(self.recv[me].data_ptr())
            sd.update_boundary()

    def op(self, name, arg, me):
        sd = self.sds[me]
        if name == "check_solve":
            sd.check_and_solve_launch()
            return sd.local_residual_wait()
        if name == "solve":
            sd.local_solve()
        elif name == "restrict":
            sd.restrict()
        elif name == "stats":
            return sd.last_inner_stats()
        elif name == "maxit":
            sd.set_local_max_iters(arg)
        elif name == "put_y":
            self.put(me, 2, 0.1 * np.random.default_rng(arg).standard_normal(sd.local_size_x) if arg else
                     np.zeros(sd.local_size_x))
        elif name == "put_b":
            self.put(me, 1, self.b[me] if arg else np.zeros(sd.local_size_x))
        elif name in ("precision", "sym"):
            if name == "precision":
                sd.set_local_precision(getattr(self.schwz.capi, "PRECISION_" + arg))
            else:
                sd.set_sym_solver(getattr(self.schwz.capi, "SYM_" + arg))
            return sd.local_precision(), sd.sym_solver(), sd.early_pack_ok()
        else:
            raise KeyError(name)
        return None

    def run(self, script):
        """script: [(name, arg, env)]; "step" = exchange, check_and_solve, wait, restrict, recorded as two ops."""
        rec = []
        for name, arg, env in script:
            with cc.upload_env(dict(self.env, **env)):
                if name == "step":
                    self.exchange()
                    self._record(rec, "check_solve", [self.op("check_solve", None, me) for me in range(self.P)])
                    self.flavours.append([sd.cg_flavour() for sd in self.sds])
                    self._record(rec, "restrict", [self.op("restrict", None, me) for me in range(self.P)])
                else:
                    self._record(rec, name, [self.op(name, arg, me) for me in range(self.P)])
        return rec

    def _record(self, rec, name, returned):
        self.torch.cuda.synchronize()
        self.forms.append([sd.y_form() for sd in self.sds])
        self.flavours_after.append([sd.cg_flavour() for sd in self.sds])
        ys = [self.get(me, 2) for me in range(self.P)]
        xs = [self.get(me, 0) for me in range(self.P)]
        assert all(np.isfinite(v).all() for v in ys + xs), name
        rec.append(dict(op=name, ret=returned, y=[digest(v) for v in ys], x=[digest(v) for v in xs],
                        y_is_x=[np.array_equal(a, b) for a, b in zip(ys, xs)], y_any=[bool(v.any()) for v in ys],
                        y_is_x_interior=[np.array_equal(a[:sd.local_size], b[:sd.local_size])
                                         for sd, a, b in zip(self.sds, ys, xs)],
                        x_any=[bool(v.any()) for v in xs]))


def digest(v):
    return hashlib.blake2b((v + 0.0).tobytes(), digest_size=16).hexdigest()


def same(a, b, what):
    assert len(a) == len(b)
    x_differs = False
    for i, (p, q) in enumerate(zip(a, b)):
        assert p["op"] == q["op"]
        where = "%s: op %d (%s)" % (what, i, p["op"])
        x_differs = p["op"] != "restrict" and (x_differs or p["op"] == "put_y")
        assert p["ret"] == q["ret"], (where, p["ret"], q["ret"])
        for me in range(len(p["y"])):
            assert p["y"][me] == q["y"][me], where + " y"
            # From a write into y to the next restriction the two forms differ in x~ by design: in state A of the
            # unified form y IS x~, so the write lands in both (and the solve behind it leaves that buffer alone),
            # while a y of its own leaves x~ as it was.  (Both take the written y for x~ in the next check residual,
            # so norms and y stay comparable.)  The restriction makes x~ = y in both.
            if not x_differs:
                assert p["x"][me] == q["x"][me], where + " x~"


def S(name, arg=None, **env):
    return (name, arg, env)


# ---- past128: one script, three sets of switches -------------------------------------------------------------------
# (slices of the script are what the tests below speak about; one subdomain serves them all: its upload takes
# longer than everything else here)
P128_SCRIPT = (
    [S("restrict"), S("put_y", 7)]                                        # 0-1   restrict before any solve
    + [S("step")] * 4                                                     # 2-9   four steps
    + [S("solve"), S("solve"), S("restrict")]                             # 10-12 solve, solve, restrict
    + [S("solve"), S("stats"), S("restrict"), S("restrict")]              # 13-16 y read without restrict; restrict twice
    + [S("put_y", 8), S("step")]                                          # 17-19 put into y between two steps
    + [S("step", SCHWZ_CG_DEFERX="0"), S("step")]                         # 20-23 a solve that does not defer x in between
    + [S("check_solve"), S("check_solve"), S("stats"), S("restrict")]     # 24-27 a discarded solve, with norms
    + [S("maxit", 40), S("step"), S("stats"), S("maxit", K)]              # 28-32 two full rings before the last x update
    + [S("put_b", 0), S("put_y", 0), S("check_solve"), S("stats"), S("restrict"), S("put_b", 1)]   # 33-38 zero rhs, y = 0
    + [S("step"), S("stats")]                                             # 39-41 ... and the next solve
    + [S("step", SCHWZ_CG_SWEEPSTART="0"), S("stats")]                    # 42-44 a start outside the walk
)


@pytest.fixture(scope="module")
def past128(schwz, torch_cuda):
    out = {}
    for key, env in (("unified", {}), ("separate", FUSE0), ("nofold", FOLD0)):
        rig = Rig(schwz, torch_cuda, PAST128, 1, env)
        out[key] = (rig.run(P128_SCRIPT), rig.forms, rig.flavours)
        del rig
    return out


def test_unified_form_equals_two_buffer_form_step_by_step(past128):
    """4 steps of check_and_solve_launch / local_residual_wait / restrict with 10 inner iterations: x~, y and the norm
    after every call equal those of SCHWZ_RESTRICT_FUSE=0; after each restrict vector(2) holds what vector(0)
    holds; the unified run really was unified (state B after a solve, A after a restriction) with flavour 254."""
    (u, uf, ufl), (s, sf, _) = past128["unified"], past128["separate"]
    same(u[:10], s[:10], "steps")
    for i in range(2, 10):
        assert sf[i] == [0]
        assert uf[i] == ([2] if u[i]["op"] == "check_solve" else [1]), (i, uf[i])
        if u[i]["op"] == "restrict":
            assert u[i]["y_is_x"] == [True] and s[i]["y_is_x"] == [True]
    assert all(f == [254] for f in ufl[:4]), ufl
    # (the steps do something)
    assert u[2]["ret"][0] > u[8]["ret"][0] > 0.0


def test_unified_form_sequences(past128):
    """Restrict before any solve; solve, solve, restrict; y read after a solve that is not restricted; restrict
    twice; a write into y between two steps; a solve with SCHWZ_CG_DEFERX=0 between two unified ones (the form
    changes for that solve and back: one copy each way); a discarded solve followed by another check-and-solve."""
    (u, uf, ufl), (s, _, _) = past128["unified"], past128["separate"]
    same(u[:28], s[:28], "sequences")
    assert uf[0] == [1] and uf[10] == [2] and uf[11] == [2] and uf[12] == [1]
    # the write into y between two steps: into x~ as well where they are one buffer, into y alone otherwise
    assert u[17]["op"] == "put_y" and u[17]["y_is_x"] == [True] and s[17]["y_is_x"] == [False]
    assert s[17]["x"] == s[16]["x"]
    assert uf[15] == [1] and uf[16] == [1]
    # x~ is untouched by solves that were not restricted, in both forms
    for r in (u, s):
        assert r[10]["x"] == r[9]["x"] and r[11]["x"] == r[9]["x"]
        assert r[11]["y"] != r[10]["y"]
        assert r[12]["x"] == r[11]["y"]
        assert r[13]["ret"] == [None] and r[14]["ret"][0][0] == K
        # the discarded solve: the second check norm is x~'s, i.e. the first one again -- from another kernel, which
        # sums the 2.1 M squares in another order (each sum within n eps / 2 ~ 2.4e-10 of the exact one, relative)
        assert r[25]["ret"][0] != 0.0 and abs(r[25]["ret"][0] - r[24]["ret"][0]) <= 5e-10 * r[24]["ret"][0]
        assert r[24]["x"] == r[23]["x"] and r[25]["x"] == r[23]["x"] and r[27]["x"] == r[25]["y"]
    # the solve without the deferred x update ran in the separate form, the next one unified again
    assert uf[20] == [0] and uf[21] == [0] and uf[22] == [2] and uf[23] == [1]
    assert ufl[5][0] & 4 == 0 and ufl[6] == [254]


def test_forty_iterations_flush_two_full_rings_out_of_place(past128):
    (u, _, _), (s, _, _), (f, _, _) = past128["unified"], past128["separate"], past128["nofold"]
    same(u[28:33], s[28:33], "40 iterations")
    same(u[28:33], f[28:33], "40 iterations, init fold")
    assert u[31]["ret"][0][0] == 40


def test_init_fold_equals_separate_launch(past128):
    """Default against SCHWZ_CG_INITFOLD=0 over the whole script: check norms, last_inner_stats and y."""
    (u, _, ufl), (f, _, ffl) = past128["unified"], past128["nofold"]
    same(u, f, "init fold")
    assert ufl == ffl


def test_init_fold_zero_residual_and_the_solve_after_it(past128):
    """b = 0 and y = 0: norm 0, no iteration, y unchanged, no NaN -- and the next solve does not see that state."""
    for key in ("unified", "separate", "nofold"):
        r = past128[key][0]
        assert r[35]["op"] == "check_solve" and r[35]["ret"] == [0.0]
        assert r[36]["ret"][0][0] == 0 and r[36]["ret"][0][1] == 0.0
        assert r[35]["y_any"] == [False] and r[37]["x_any"] == [False]
        assert r[39]["ret"][0] > 0.0 and r[41]["ret"][0][0] == K and np.isfinite(r[41]["ret"][0][1])
        assert r[40]["y_any"] == [True]
    same(past128["unified"][0][33:42], past128["separate"][0][33:42], "zero rhs")


def test_start_outside_the_walk(past128):
    """SCHWZ_CG_SWEEPSTART=0: the chunk-by-chunk start launch and cg_init_finalize_kernel, with either value of
    SCHWZ_CG_INITFOLD, and the out-of-place x update behind it."""
    (u, uf, ufl), (s, _, sfl), (f, _, _) = past128["unified"], past128["separate"], past128["nofold"]
    same(u[42:], s[42:], "no walk start")
    same(u[42:], f[42:], "no walk start, init fold")
    assert ufl[-1][0] & 32 == 0 and ufl[-1][0] & 4 == 4 and ufl[-1] == sfl[-1]
    assert uf[42] == [2] and u[44]["ret"][0][0] == K


# ---- the flush forms on an odd number of rows ----------------------------------------------------------------------

SMALL_SCRIPT = ([S("put_y", 3)] + [S("step")] * 3 + [S("solve"), S("solve"), S("restrict")]
                + [S("maxit", 40), S("step"), S("stats"), S("maxit", 0), S("step"), S("maxit", K), S("step")])


@pytest.mark.parametrize("variant", [0, 6], ids=["row_pairs", "stored_q"])
def test_out_of_place_flush_on_odd_rows(schwz, torch_cuda, variant):
    """5 x 7 x 9 (315 rows: the odd-row tail) with SCHWZ_CG_DEFERX=2, the q-free and the stored-q iteration
    (spmv_variant 6), 10, 40 and 0 iterations, each against SCHWZ_RESTRICT_FUSE=0."""
    env = {"SCHWZ_CG_DEFERX": "2"}
    a = Rig(schwz, torch_cuda, SMALL, 1, env, spmv_variant=variant)
    b = Rig(schwz, torch_cuda, SMALL, 1, dict(env, **FUSE0), spmv_variant=variant)
    assert a.sds[0].local_size_x % 2 == 1
    ra, rb = a.run(SMALL_SCRIPT), b.run(SMALL_SCRIPT)
    same(ra, rb, "odd rows")
    assert all(f[0] & 4 for f in a.flavours) and a.flavours == b.flavours
    if variant == 6:
        assert all(f[0] & 3 == 0 for f in a.flavours), a.flavours
    assert all(f == [0] for f in b.forms)
    assert a.forms[0] == [1] and a.forms[1] == [2] and a.forms[2] == [1]
    assert ra[1]["ret"][0] > ra[5]["ret"][0] > 0.0
    assert ra[13]["op"] == "stats" and ra[13]["ret"][0][0] == 40


# ---- a switch of the local solver inside the state machine of the forms ----------------------------------------------

SWITCH_SCRIPT = (
    [S("put_y", 3), S("step"), S("step")]                                                  # CG, state A
    + [S("sym", "CHEBYSHEV"), S("step"), S("stats"), S("solve"), S("solve"), S("restrict")]   # switched in state A
    + [S("sym", "CG"), S("step"), S("stats")]
    + [S("check_solve"), S("sym", "CHEBYSHEV"), S("check_solve"), S("stats"), S("restrict")]  # switched in state B
    + [S("sym", "CG"), S("check_solve"), S("precision", "F32"), S("step"), S("stats"), S("solve")]   # state B again
    + [S("precision", "F64"), S("check_solve"), S("check_solve"), S("restrict"), S("step"), S("stats")]
)


def switch_kinds(script):
    """The solver selected after every recorded operation of `script` ("step" records two)."""
    kinds, kind = [], "CG"
    for name, arg, _ in script:
        if name == "sym":
            kind = arg
        elif name == "precision":
            kind = "F32" if arg == "F32" else "CG"
        kinds += [kind] * (2 if name == "step" else 1)
    return kinds


@pytest.mark.parametrize("P", [1, 2])
def test_switching_the_local_solver_in_either_form(schwz, torch_cuda, P):
    """5 x 7 x 9 with SCHWZ_CG_DEFERX=2 (one subdomain: unified form), CG -> Chebyshev -> CG -> Chebyshev -> CG ->
    fp32 -> CG with the switches in state A and in state B (behind a discarded solve), against
    SCHWZ_RESTRICT_FUSE=0: no arithmetic depends on where y lives, so every returned value, y and x~ are equal bit for
    bit.  While Chebyshev or the fp32 CG is selected y has a vector of its own and there is no flavour; a CG solve of
    one subdomain leaves state B, its restriction state A; every solver reports its K iterations; with two subdomains
    the restriction after an in-place solve copies y (a swap would bring in a buffer no solve has written)."""
    env = {"SCHWZ_CG_DEFERX": "2"}
    a = Rig(schwz, torch_cuda, SMALL, P, env)
    b = Rig(schwz, torch_cuda, SMALL, P, dict(env, **FUSE0))
    ra, rb = a.run(SWITCH_SCRIPT), b.run(SWITCH_SCRIPT)
    same(ra, rb, "switches, P = %d" % P)
    kinds = switch_kinds(SWITCH_SCRIPT)
    assert len(kinds) == len(ra) and {"CG", "CHEBYSHEV", "F32"} == set(kinds)
    cg_solve = False   # the last solve was a CG solve (and no switch since)
    for i, (r, kind) in enumerate(zip(ra, kinds)):
        where = (i, r["op"], kind)
        if r["op"] in ("sym", "precision"):
            want = (int(kind == "F32"), int(kind == "CHEBYSHEV"), kind == "CG" and P > 1)
            assert r["ret"] == [want] * P and rb[i]["ret"] == [want] * P, where
            cg_solve = False
        if r["op"] in ("check_solve", "solve"):
            cg_solve = kind == "CG"
        if kind != "CG":
            for rig in (a, b):
                assert rig.forms[i] == [0] * P and rig.flavours_after[i] == [0] * P, where
        elif P == 1 and r["op"] == "check_solve":
            assert a.forms[i] == [2] and a.flavours_after[i][0] & 4, where
        elif P == 1 and r["op"] == "restrict" and cg_solve:
            assert a.forms[i] == [1], where
        if r["op"] == "stats":
            assert [it for it, _ in r["ret"]] == [K] * P, where
        if r["op"] == "restrict":
            assert r["y_is_x_interior"] == [True] * P and rb[i]["y_is_x_interior"] == [True] * P, where
    assert all(f == [0] * P for f in b.forms)
    assert sum(r["op"] == "restrict" and k != "CG" for r, k in zip(ra, kinds)) == 4
    # (the steps do something, with every solver)
    norms = [r["ret"][0] for r in ra if r["op"] == "check_solve"]
    assert norms[0] > norms[2] > 0.0 and all(v > 0.0 for v in norms)


# ---- with neighbours nothing changes -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def slabs(schwz, torch_cuda):
    out = {}
    script = [S("step")] * 3 + [S("stats")]
    for key, env in (("default", {}), ("separate", FUSE0), ("nofold", FOLD0)):
        # (some 850 k rows a slab: below the sizes from which x is deferred and the matrix walks by default, so the
        # switches that do both at every size)
        rig = Rig(schwz, torch_cuda, SLABS, 3, dict(env, SCHWZ_CG_DEFERX="2", SCHWZ_SPMV_SWEEP="2"))
        out[key] = (rig.run(script), rig.forms, rig.flavours)
        del rig
    return out


def test_with_neighbours_the_separate_form_stays(slabs):
    (d, df, dfl), (s, sf, sfl) = slabs["default"], slabs["separate"]
    same(d, s, "slabs")
    assert all(f == [0, 0, 0] for f in df) and all(f == [0, 0, 0] for f in sf)
    assert dfl == sfl
    assert d[0]["ret"][1] > d[4]["ret"][1] > 0.0


def test_init_fold_on_the_dual_start_launch(slabs):
    """Subdomains with overlap: the start walk also leaves the check norm of x~ in a third bank."""
    (d, _, dfl), (f, _, ffl) = slabs["default"], slabs["nofold"]
    same(d, f, "slabs, init fold")
    assert dfl == ffl
    assert all(fl & 32 for step in dfl for fl in step), dfl
    assert d[6]["ret"][0][0] == K
