"""The vector passes of the outer FGMRES on a single-basis object (csrc/outer.hip, the *_f32 kernels: V in fp32, a lane
on four rows) against np.longdouble references, at the bounds tests/test_gpu_outer_kernels.py derives.  The widened
fp32 columns are exact inputs of an fp64 computation, so those bounds carry over unchanged:

  dots            |err| <= g(n) * sum_r |V_i[r] w[r]|,  g(n) = n u / (1 - n u), u = 2^-53
  projected rows  |err_r| <= (j + 3) 2^-52 (|w_r| + sum_i |h_i V_i[r]|)
  residual        the bits of numpy's b - t;  |w . w - ref| <= g(n) sum_r w_r^2

Sizes: n = 1, 2, 3, 5 (a lone lane's tail of one, two, three rows and one row past a full lane), 63 / 64 / 65 and
255 / 257, 4099 (several workgroups) and 1024 * 1024 + 1031: past the 1024 x 256 x 4 rows one trip of the capped grid
covers, no multiple of 4.  j = 0, 1, 7, 29 on a restart-30 object: one, one, one and four register blocks; j = 39 on a
restart-40 object at n = 257 and 4099: more than 32 columns, the subtraction complete before the first dot.  Entries
have mixed magnitudes (2^-20 .. 2^20).  The columns are placed with basis_write and read back with basis_read, which
are tested first against x.astype(float32).astype(float64)."""
import numpy as np
import pytest

import stream_rig as rig
from test_gpu_outer_kernels import LD, check_dots, gamma

pytestmark = pytest.mark.gpu
BIG = 1024 * 1024 + 1031
SIZES = [1, 2, 3, 5, 63, 64, 65, 255, 257, 4099, BIG]
JS = [0, 1, 7, 29]
RESTART = 30
CASES = [(n, j, RESTART) for n in SIZES for j in JS] + [(257, 39, 40), (4099, 39, 40)]

_data, _objs = {}, {}


def rounded(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def mixed(rng, shape):
    return rng.standard_normal(shape) * 2.0 ** rng.integers(-20, 21, size=shape)


def data(n, restart=RESTART):
    """(V: restart + 1 columns in float64, not yet rounded; w; b; t; h: restart coefficients): computed once, read-only."""
    if (n, restart) not in _data:
        rng = np.random.default_rng(2000 + n % 997 + restart)
        out = (mixed(rng, (restart + 1, n)), mixed(rng, n), mixed(rng, n), mixed(rng, n),
               rng.standard_normal(restart) * 2.0 ** rng.integers(-8, 9, size=restart))
        for a in out:
            a.setflags(write=False)
        _data[(n, restart)] = out
    return _data[(n, restart)]


def dev(torch, host):
    return torch.from_numpy(np.array(host, dtype=np.float64)).cuda()  # (a copy: the shared inputs are read-only)


def put(schwz, torch, host, ptr, stream=0):
    t = dev(torch, host)
    schwz.outer_copy(len(host), t.data_ptr(), ptr, stream)
    torch.cuda.synchronize()


def get(schwz, torch, ptr, n):
    t = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    schwz.outer_copy(n, ptr, t.data_ptr())
    torch.cuda.synchronize()
    return t.cpu().numpy()[:n]


def read_column(torch, o, j):
    t = torch.full((o.n + 2,), -3.0, dtype=torch.float64, device="cuda")
    o.basis_read(j, 0, o.n, t.data_ptr() + 8)
    torch.cuda.synchronize()
    host = t.cpu().numpy()
    assert host[0] == -3.0 and host[-1] == -3.0
    return host[1:-1]


def outer_with_basis(schwz, torch, n, restart=RESTART, basis="single"):
    """One schwz_outer per (size, restart, basis) with V_0 .. V_(restart-1) placed by basis_write (the tests rewrite w,
    V_restart and V_0, and put V_0 back)."""
    key = (n, restart, basis)
    if key not in _objs:
        V = data(n, restart)[0]
        o = schwz.Outer(n, restart) if basis is None else schwz.Outer(n, restart, basis)
        for i in range(restart):
            o.basis_write(i, 0, n, dev(torch, V[i]).data_ptr())
        torch.cuda.synchronize()
        _objs[key] = o
    return _objs[key]


# ---- basis_write / basis_read -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("first", [0, 1, 3, 64, 65])
@pytest.mark.parametrize("n", [65, 70, 4099, BIG])
def test_basis_write_then_read(schwz, torch_cuda, n, first, shift):
    """Rows [first, first + count) of V_1 for count = 0, 1 and up to the end; the fp64 side 16-byte aligned and 8 bytes
    off.  The rows outside, the neighbouring columns and the memory around the destination keep their sentinels."""
    torch = torch_cuda
    rng = np.random.default_rng(n + 7 * first + shift)
    o = schwz.Outer(n, 2, "single")
    base = {j: mixed(rng, n) for j in (0, 1, 2)}
    for j in (0, 1, 2):
        o.basis_write(j, 0, n, dev(torch, base[j]).data_ptr())
    for count in sorted({0, min(1, n - first), n - first}):  # (first = n = 65: the empty range at the end)
        x = mixed(rng, count + 2)
        src = dev(torch, x)
        o.basis_write(1, first, count, src.data_ptr() + 8 * shift)
        want = rounded(base[1])
        want[first:first + count] = rounded(x[shift:shift + count])
        assert read_column(torch, o, 1).tobytes() == want.tobytes(), (n, first, count)
        assert read_column(torch, o, 0).tobytes() == rounded(base[0]).tobytes()
        assert read_column(torch, o, 2).tobytes() == rounded(base[2]).tobytes()
        dst = torch.full((count + 3,), -9.0, dtype=torch.float64, device="cuda")
        o.basis_read(1, first, count, dst.data_ptr() + 8 * (1 + shift))
        torch.cuda.synchronize()
        host = dst.cpu().numpy()
        assert host[1 + shift:1 + shift + count].tobytes() == want[first:first + count].tobytes()
        assert (host[:1 + shift] == -9.0).all() and (host[1 + shift + count:] == -9.0).all()
        base[1] = want


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_basis_write_then_read_tiny(schwz, torch_cuda, n):
    torch = torch_cuda
    rng = np.random.default_rng(n)
    o = schwz.Outer(n, 1, "single")
    x = mixed(rng, n)
    o.basis_write(1, 0, n, dev(torch, x).data_ptr())
    assert read_column(torch, o, 1).tobytes() == rounded(x).tobytes()
    assert read_column(torch, o, 0).tobytes() == np.zeros(n).tobytes()
    o.basis_write(1, n - 1, 1, dev(torch, [5.0]).data_ptr())
    assert read_column(torch, o, 1).tobytes() == np.append(rounded(x)[:n - 1], 5.0).tobytes()


def test_rounding_is_to_nearest_even(schwz, torch_cuda):
    torch = torch_cuda
    x = np.array([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, -(1.0 + 2.0 ** -24), 2.0 ** -140,
                  1e39, -1e39, 0.0, -0.0, 3.0])
    o = schwz.Outer(len(x), 1, "single")
    o.basis_write(0, 0, len(x), dev(torch, x).data_ptr())
    with np.errstate(over="ignore"):
        assert read_column(torch, o, 0).tobytes() == rounded(x).tobytes()


def test_read_and_write_are_plain_copies_on_a_double_basis(schwz, torch_cuda):
    torch = torch_cuda
    n = 261
    x = mixed(np.random.default_rng(1), n)
    o = schwz.Outer(n, 2, "double")
    o.basis_write(1, 3, n - 3, dev(torch, x).data_ptr() + 8)
    assert get(schwz, torch, o.vector(o.V, 1), n).tobytes() == np.append(np.zeros(3), x[1:n - 2]).tobytes()
    assert read_column(torch, o, 1).tobytes() == np.append(np.zeros(3), x[1:n - 2]).tobytes()
    assert (get(schwz, torch, o.vector(o.V, 0), n) == 0.0).all() and (get(schwz, torch, o.vector(o.V, 2), n) == 0.0).all()


def test_ranges_out_of_bounds_are_invalid(schwz, torch_cuda):
    torch = torch_cuda
    o = schwz.Outer(10, 2, "single")
    t = torch.zeros(16, dtype=torch.float64, device="cuda")
    for call in (o.basis_read, o.basis_write):
        for j, first, count in ((3, 0, 1), (-1, 0, 1), (0, -1, 1), (0, 0, 11), (0, 5, 6), (0, 11, 0), (0, 0, -1)):
            with pytest.raises(schwz.SchwzError) as e:
                call(j, first, count, t.data_ptr())
            assert e.value.code == schwz.capi.ERR_INVALID
    o.basis_read(0, 10, 0, t.data_ptr())
    with pytest.raises(schwz.SchwzError) as e:
        o.vector(o.V, 0)
    assert e.value.code == schwz.capi.ERR_INVALID
    for which in (o.Z, o.W, o.B):
        assert o.vector(which, 0)
    with pytest.raises(schwz.SchwzError):
        schwz.Outer(10, 2, "half")


# ---- the passes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,j,restart", CASES)
def test_dots(schwz, torch_cuda, n, j, restart):
    V, w = data(n, restart)[:2]
    V = rounded(V)
    o = outer_with_basis(schwz, torch_cuda, n, restart)
    put(schwz, torch_cuda, w, o.vector(o.W))
    got = o.dots(j)
    assert got.shape == (j + 2,)
    check_dots(got, V, w, j, n)
    again = o.dots(j)
    assert got.tobytes() == again.tobytes()  # fixed order of every sum: the same bits
    assert get(schwz, torch_cuda, o.vector(o.W), n).tobytes() == w.tobytes()  # w is only read


@pytest.mark.parametrize("n,j,restart", CASES)
def test_project_dots(schwz, torch_cuda, n, j, restart):
    V, w, _, _, h = data(n, restart)
    V = rounded(V)
    o = outer_with_basis(schwz, torch_cuda, n, restart)
    put(schwz, torch_cuda, w, o.vector(o.W))
    got = o.project_dots(j, h[:j + 1])
    new = get(schwz, torch_cuda, o.vector(o.W), n)
    terms = h[:j + 1, None].astype(LD) * V[:j + 1].astype(LD)
    ref = w.astype(LD) - terms.sum(axis=0)
    bound = (j + 3) * 2.0 ** -52 * (np.abs(w) + np.abs(terms).sum(axis=0).astype(np.float64))
    err = np.abs((new.astype(LD) - ref).astype(np.float64))
    assert (err <= bound).all(), (n, j, float((err / np.maximum(bound, 1e-300)).max()))
    # the dots are those of the w the pass stored
    check_dots(got, V, new, j, n)
    put(schwz, torch_cuda, w, o.vector(o.W))
    again = o.project_dots(j, h[:j + 1])
    assert got.tobytes() == again.tobytes()
    assert get(schwz, torch_cuda, o.vector(o.W), n).tobytes() == new.tobytes()
    # the columns are only read
    for i in (0, j):
        assert read_column(torch_cuda, o, i).tobytes() == V[i].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_start_and_normalize_store_the_rounded_product(schwz, torch_cuda, n):
    """fl32(w * s): the bits of (w * s).astype(float32).  V_30 and V_0 are written, V_0 is put back."""
    V, w = data(n)[:2]
    o = outer_with_basis(schwz, torch_cuda, n)
    put(schwz, torch_cuda, w, o.vector(o.W))
    o.normalize(RESTART - 1, 0.3)
    assert read_column(torch_cuda, o, RESTART).tobytes() == rounded(w * 0.3).tobytes()
    o.start(1.0 / 7.0)
    assert read_column(torch_cuda, o, 0).tobytes() == rounded(w * (1.0 / 7.0)).tobytes()
    assert read_column(torch_cuda, o, 1).tobytes() == rounded(V[1]).tobytes()  # the neighbouring columns are intact
    assert read_column(torch_cuda, o, RESTART - 1).tobytes() == rounded(V[RESTART - 1]).tobytes()
    assert get(schwz, torch_cuda, o.vector(o.W), n).tobytes() == w.tobytes()
    o.basis_write(0, 0, n, dev(torch_cuda, V[0]).data_ptr())
    torch_cuda.cuda.synchronize()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n,basis", [(n, "single") for n in SIZES] + [(n, "double") for n in (1, 65, 4099)])
def test_residual(schwz, torch_cuda, n, shift, basis):
    """w = b - t with t 16-byte aligned and 8 bytes off; the double-basis object runs the same kernel."""
    torch = torch_cuda
    _, w, b, t, _ = data(n)
    o = outer_with_basis(schwz, torch, n, basis=basis)
    put(schwz, torch, b, o.vector(o.B))
    put(schwz, torch, w, o.vector(o.W))
    td = dev(torch, np.append(np.full(shift, 7.0), t))
    ww = o.residual(td.data_ptr() + 8 * shift)
    new = get(schwz, torch, o.vector(o.W), n)
    assert new.tobytes() == (b - t).tobytes()
    ref = np.sum(new.astype(LD) ** 2)
    assert abs(float(LD(ww) - ref)) <= gamma(n) * float(ref), (n, ww, float(ref))
    assert o.residual(td.data_ptr() + 8 * shift) == ww
    assert get(schwz, torch, o.vector(o.B), n).tobytes() == b.tobytes()


@pytest.mark.parametrize("n,j", [(65, 7), (4099, 29), (1024 * 512 + 1031, 1)])
def test_create_basis_double_is_create(schwz, torch_cuda, n, j):
    """schwz_outer_create_basis(.., 0, ..) and schwz_outer_create on the same data: the same bytes from dots and
    project_dots, in w as well."""
    V, w, _, _, h = data(n)
    res = []
    for basis in (None, "double"):
        o = schwz.Outer(n, RESTART, basis)
        for i in range(j + 1):
            put(schwz, torch_cuda, V[i], o.vector(o.V, i))
        put(schwz, torch_cuda, w, o.vector(o.W))
        a = o.dots(j)
        b = o.project_dots(j, h[:j + 1])
        res.append((a.tobytes(), b.tobytes(), get(schwz, torch_cuda, o.vector(o.W), n).tobytes()))
        o.close()
    assert res[0] == res[1]


def test_on_a_stream(schwz, torch_cuda):
    """Every call of the single-basis object on a non-default stream that a delay holds shut while the calls are issued,
    its inputs poisoned until the gate has passed (stream_rig.py), against the same calls on the default stream, bit
    for bit.  dots, project_dots and residual read back and so synchronise by contract."""
    torch = torch_cuda
    n, j = 4099, 9
    V, w, b, t, h = data(n)

    def body(r):
        o = r.hold(schwz.Outer(n, RESTART, "single"))
        cols = [r.input(V[i]) for i in range(j + 1)]
        d_w, d_b, d_t = r.input(w), r.input(b), r.input(t)
        r.arm()
        for i, c in enumerate(cols):
            r.call(o.basis_write, i, 0, n, c.data_ptr(), stream=r.handle)
        r.call(schwz.outer_copy, n, d_w.data_ptr(), o.vector(o.W), stream=r.handle)
        r.call(schwz.outer_copy, n, d_b.data_ptr(), o.vector(o.B), stream=r.handle)
        r.call(o.normalize, j, 0.3, stream=r.handle)
        r.call(o.start, 1.0 / 7.0, stream=r.handle)
        back = r.output(n)
        r.call(o.basis_read, j + 1, 0, n, back.data_ptr(), stream=r.handle)
        r.snap(back)
        h1 = r.call(o.dots, j, stream=r.handle, reads_back=True)
        h2 = r.call(o.project_dots, j, h[:j + 1], stream=r.handle, reads_back=True)
        ww = r.call(o.residual, d_t.data_ptr(), stream=r.handle, reads_back=True)
        new = r.output(n)
        r.call(schwz.outer_copy, n, o.vector(o.W), new.data_ptr(), stream=r.handle, reads_back=True)
        r.snap(new)
        return [h1, h2, np.array([ww])]

    (back, new), host = rig.both(torch, body, "single-basis outer passes")
    assert back[:n].tobytes() == rounded(w * 0.3).tobytes()
    assert new[:n].tobytes() == (b - t).tobytes()
    Vr = rounded(V)
    Vr[0] = rounded(w * (1.0 / 7.0))
    check_dots(host[0], Vr, w, j, n)
