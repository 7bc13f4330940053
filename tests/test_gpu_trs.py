"""The triangular-solve kernels of csrc/trs.hip (one-workgroup kernel, level plan with wide and narrow
segments and its hipGraph replay, flag-driven sweeps with a lane or a wave per row) and the Jacobi-sweep solves
of csrc/parilu.hip, on factors built in numpy -- no factorisation routine of the library stands between the
test and the kernel -- at the thresholds where the dispatch changes and on the structures at the ends of the
range: no dependency at all, one single chain, levels exactly at the wide/narrow limit, rows at and beyond one
wave, badly scaled pivots.

Every case solves twice with different right-hand sides (the flag vectors must have been reset), once in place,
and must satisfy |y - y_ref| <= 2 * bound componentwise, where y_ref is the substitution in longdouble and
bound the forward-error bound of substitution in float64 for ANY summation order (hp_reference.trs_error_bound,
Higham Thm 8.5 with the comparison matrix).  The factor 2 covers the reference's own rounding and the
second-order terms the theorem drops.  The bound is derived; nothing in it is measured on the kernels.
Paths that claim to sum every row in CSR order (lane-per-row flag sweep, level and narrow kernels) must also
agree bit for bit; the wave-per-row sweep sums by butterfly and the one-workgroup kernel makes no such claim,
so they get the bound only.

Not tested: the timeout branch of the flag sweeps (a wait beyond 3 s gives up with NaN and *err = 1).  Driving a
sweep into it means stalling a persistent kernel on a shared GPU on purpose.  The longest chain here (20 000
rows, about 2 us per hop) stays four orders of magnitude below that limit."""
import numpy as np
import pytest

import hp_reference as hp

pytestmark = pytest.mark.gpu

LD = np.longdouble
RATIOS = []   # (case, max err / bound): read by tools/hp_reference_probe.py


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _make(schwz, f, perms):
    args = (f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"])
    if perms is None:
        return schwz.Trs(*args)
    if perms[0] is perms[1]:
        return schwz.Trs(*args, perms[0])
    return schwz.TrsLU(*args, perms[0], perms[1])


def _solve(torch, t, b, in_place=False):
    d_b = _dev(torch, b)
    d_y = d_b if in_place else torch.full((len(b),), float("nan"), dtype=torch.float64, device="cuda")
    t.solve(d_b.data_ptr(), d_y.data_ptr())
    torch.cuda.synchronize()
    return d_y.cpu().numpy()


class Reference:
    def __init__(self, f, perms):
        self.L, self.U = hp.factors(f)
        self.pin, self.pout = (None, None) if perms is None else perms

    def check(self, b, y, tag):
        y_ref, w1, w0 = hp.trs_apply(self.L, self.U, self.pin, self.pout, b, parts=True)
        e = hp.trs_error_bound(self.L, self.U, w1, w0)
        bound = e
        if self.pout is not None:
            bound = np.zeros_like(e)
            bound[np.asarray(self.pout, dtype=np.int64)] = e
        assert np.isfinite(y).all(), tag
        err = np.abs(y.astype(LD) - y_ref)
        worst = float((err / np.maximum(bound, np.finfo(LD).tiny)).max()) if len(y) else 0.0
        RATIOS.append((tag, worst))
        print("%s: max err / bound %.3f, max rel err %.2e" % (tag, worst, float(err.max() / np.abs(y_ref).max())))
        assert (err <= 2 * bound).all(), (tag, worst)


def _case(schwz, torch, f, perms, tag, seed=0, ref=None):
    """Two right-hand sides, then the first in place; the bound on both.  Returns the two results."""
    n = len(f["l_rp"]) - 1
    rng = np.random.default_rng(1000 + seed)
    b1, b2 = rng.standard_normal(n), rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-8, 9, n))
    t = _make(schwz, f, perms)
    y1 = _solve(torch, t, b1)
    y2 = _solve(torch, t, b2)
    assert np.array_equal(_solve(torch, t, b1, in_place=True), y1), tag + ": in place"
    assert np.array_equal(_solve(torch, t, b1), y1), tag + ": third solve"
    ref = ref or Reference(f, perms)
    ref.check(b1, y1, tag + " rhs 1")
    ref.check(b2, y2, tag + " rhs 2")
    t.close()
    return (y1, y2), ref


def _same_bits(a, b, tag):
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), "%s: rhs %d differs in %d entries" % (tag, k + 1, int((u != v).sum()))


def _flags_and_plan(schwz, torch, monkeypatch, f, perms, tag, seed=0, same_bits=True):
    """The default dispatch and the level plan (SCHWZ_TRS_FLAGS=0): the bound on both, the same bits where both
    sum in CSR order."""
    monkeypatch.delenv("SCHWZ_TRS_FLAGS", raising=False)
    ya, ref = _case(schwz, torch, f, perms, tag + " default", seed)
    monkeypatch.setenv("SCHWZ_TRS_FLAGS", "0")
    yb, _ = _case(schwz, torch, f, perms, tag + " plan", seed, ref)
    monkeypatch.delenv("SCHWZ_TRS_FLAGS", raising=False)
    if same_bits:
        _same_bits(ya, yb, tag + ": flags vs plan")
    return ya


def _perm_sets(n, rng, lu=True):
    p, q = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
    return [None, (p, p)] + ([(p, q)] if lu else [])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 8191, 8192, 8193])
def test_trs_five_point_factors_around_the_one_workgroup_limit(schwz, torch_cuda, monkeypatch, n):
    """n <= 8192 with a permutation: the one-workgroup kernel.  Without one (every ILU(0)): the level plan with
    trs_narrow_kernel.  n = 8193: the lane-per-row flag sweep, the same bits as the level plan."""
    rng = np.random.default_rng(n)
    f = hp.five_point_factors(n, max(1, int(np.sqrt(n))), rng)
    for k, perms in enumerate(_perm_sets(n, rng)):
        _flags_and_plan(schwz, torch_cuda, monkeypatch, f, perms, "five-point n=%d perms %d" % (n, k), k)


def test_trs_diagonal_factors_are_one_level(schwz, torch_cuda, monkeypatch):
    n = 20000
    rng = np.random.default_rng(2)
    f = hp.diagonal_factors(n, rng)
    for k, perms in enumerate(_perm_sets(n, rng)):
        _flags_and_plan(schwz, torch_cuda, monkeypatch, f, perms, "diagonal perms %d" % k, k)


def test_trs_bidiagonal_factors_are_one_chain(schwz, torch_cuda, monkeypatch):
    """One row per level.  On the flag path every lane waits for its neighbour in the same wave: the case the
    progress argument of trs_flag_kernel has to hold for.  On the level plan: 20 000 narrow levels in one
    segment."""
    n = 20000
    rng = np.random.default_rng(3)
    f = hp.bidiagonal_factors(n, rng)
    for k, perms in enumerate(_perm_sets(n, rng)):
        _flags_and_plan(schwz, torch_cuda, monkeypatch, f, perms, "chain perms %d" % k, k)


WIDTHS = [255, 256, 257] * 12   # n = 9216 > 8192; narrow, wide, wide, narrow, ...: 24 segments per factor


def test_trs_levels_at_the_wide_narrow_limit_and_the_graph_cache(schwz, torch_cuda, monkeypatch):
    """Levels of exactly 255 (narrow), 256 and 257 (wide) rows: the segment planner; more than 8 segments: the
    plan is captured into a hipGraph per (b, y) pointer pair, four of them are cached and a fifth pair falls
    back to launch by launch."""
    torch = torch_cuda
    rng = np.random.default_rng(4)
    f = hp.layered_factors(WIDTHS, rng)
    n = sum(WIDTHS)
    L, U = hp.factors(f)
    assert [len(r) if not isinstance(p, slice) else 1 for r, p in L.plan] == WIDTHS
    assert [len(r) if not isinstance(p, slice) else 1 for r, p in U.plan] == WIDTHS
    for k, perms in enumerate(_perm_sets(n, rng, lu=False)):
        _flags_and_plan(schwz, torch, monkeypatch, f, perms, "255/256/257 perms %d" % k, k)
    # six distinct (b, y) pairs on one plan object, then the first pair again; against the flag sweep's bits
    flag = _make(schwz, f, None)
    monkeypatch.setenv("SCHWZ_TRS_FLAGS", "0")
    plan = _make(schwz, f, None)
    monkeypatch.delenv("SCHWZ_TRS_FLAGS", raising=False)
    bs = [rng.standard_normal(n) for _ in range(6)]
    pairs = [(_dev(torch, b), torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")) for b in bs]
    assert len({(b.data_ptr(), y.data_ptr()) for b, y in pairs}) == 6
    want = [_solve(torch, flag, b) for b in bs]
    Reference(f, None).check(bs[5], want[5], "255/256/257 sixth pair")
    for rounds in range(2):   # the second round replays the four cached graphs and relaunches the other two
        for (d_b, d_y), w in zip(pairs, want):
            d_y.fill_(float("nan"))
            plan.solve(d_b.data_ptr(), d_y.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(d_y.cpu().numpy(), w)
    d_b, d_y = pairs[0]
    plan.solve(d_b.data_ptr(), d_y.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_y.cpu().numpy(), want[0])


@pytest.mark.parametrize("longest", [64, 65])
def test_trs_longest_row_at_one_wave(schwz, torch_cuda, monkeypatch, longest):
    """Longest row 64: a lane per row, through Trs and TrsLU.  65: Trs falls back to the level plan, TrsLU
    takes the wave-per-row sweep (butterfly sum: the bound only)."""
    rng = np.random.default_rng(longest)
    widths = [300] * 28
    f = hp.layered_factors(widths, rng, long_row=(5, longest - 1))
    n = sum(widths)
    assert n > 8192
    assert max(np.diff(f["l_rp"]).max(), np.diff(f["u_rp"]).max()) == longest
    none, same, lu = _perm_sets(n, rng)
    _flags_and_plan(schwz, torch_cuda, monkeypatch, f, none, "longest %d Trs" % longest, 0)
    _flags_and_plan(schwz, torch_cuda, monkeypatch, f, same, "longest %d Trs perm" % longest, 1)
    _flags_and_plan(schwz, torch_cuda, monkeypatch, f, lu, "longest %d TrsLU" % longest, 2, same_bits=longest <= 64)


def test_trs_lu_banded_rows_of_several_waves(schwz, torch_cuda, monkeypatch):
    """Rows of 200 to 300 entries: the four-groups-of-64 loop of trs_flag_wave_kernel with a ragged last
    group, one row per level."""
    n = 8300
    rng = np.random.default_rng(7)
    f = hp.banded_factors(n, 200, 300, rng)
    ln = np.diff(f["l_rp"])
    assert ln.max() > 256 and (ln[400:] >= 200).all()
    _, _, lu = _perm_sets(n, rng)
    _flags_and_plan(schwz, torch_cuda, monkeypatch, f, lu, "banded TrsLU", 0, same_bits=False)


@pytest.mark.parametrize("kind", ["five_point_4000", "five_point_8193", "layered_lu"])
def test_trs_badly_scaled_pivots(schwz, torch_cuda, monkeypatch, kind):
    """Diagonals from +-[2^-20, 2^20] by signed power-of-two row and column scalings of well-conditioned
    factors: non-unit, negative pivots in L and in U; M(T) stays well conditioned up to the scalings."""
    rng = np.random.default_rng(len(kind))
    if kind == "layered_lu":
        f = hp.layered_factors([300] * 28, rng, long_row=(5, 80))
    else:
        n = int(kind.split("_")[-1])
        f = hp.five_point_factors(n, int(np.sqrt(n)), rng)
    f = hp.rescale(f, rng)
    n = len(f["l_rp"]) - 1
    for name in ("l", "u"):
        T = hp.Tri(f[name + "_rp"], f[name + "_col"], f[name + "_val"], name == "l")
        d = np.abs(T.val64[T.dpos])
        assert (f[name + "_val"] < 0).any() and d.max() / d.min() > 2.0 ** 20
    none, same, lu = _perm_sets(n, rng)
    if kind == "layered_lu":
        _flags_and_plan(schwz, torch_cuda, monkeypatch, f, lu, "scaled " + kind, 0, same_bits=False)
    else:
        _flags_and_plan(schwz, torch_cuda, monkeypatch, f, none, "scaled " + kind, 0)
        _flags_and_plan(schwz, torch_cuda, monkeypatch, f, same, "scaled " + kind + " perm", 1)


def test_jacobi_sweep_solves_past_the_grid_cap(schwz, torch_cuda):
    """trs_jacobi_kernel with n = 750^2 = 562 500 > 524 288 rows: the launch is capped and strides.  Against
    the truncated Neumann series in longdouble, within twice the componentwise bound of a float64 evaluation
    that hp_reference.jacobi_sweep_solve derives pass by pass."""
    torch = torch_cuda
    n = 750 * 750
    assert n > 2048 * 256
    rng = np.random.default_rng(9)
    f = hp.five_point_factors(n, 750, rng)
    L, U = hp.factors(f)
    b1, b2 = rng.standard_normal(n), rng.standard_normal(n)
    for sweeps in (1, 3):
        t = schwz.TrsSweeps(f["l_rp"], f["l_col"], f["l_val"], f["u_rp"], f["u_col"], f["u_val"], sweeps)
        assert t.sweeps == sweeps
        y1, y2 = _solve(torch, t, b1), _solve(torch, t, b2)
        assert np.array_equal(_solve(torch, t, b1), y1)
        for b, y in ((b1, y1), (b2, y2)):
            y_ref, bound = hp.jacobi_sweep_solve(L, U, b, sweeps, bound=True)
            err = np.abs(y.astype(LD) - y_ref)
            RATIOS.append(("jacobi sweeps %d, n = 562500" % sweeps, float((err / bound).max())))
            print("jacobi sweeps %d: max err / bound %.3f" % (sweeps, float((err / bound).max())))
            assert np.isfinite(y).all() and (err <= 2 * bound).all()
        t.close()
