"""The vector passes of the outer FGMRES (csrc/outer.hip) and schwz_ras_apply_interior against np.longdouble
references, at bounds that follow from the arithmetic, not from what the kernels give:

  dots            |err| <= g(n) * sum_r |V_i[r] w[r]|,  g(n) = n u / (1 - n u), u = 2^-53: the classical bound of a dot
                  product of length n, which holds for any order of the sum, with or without fused multiply-adds
  projected rows  |err_r| <= (j + 3) 2^-52 (|w_r| + sum_i |h_i V_i[r]|): j + 1 products and j + 1 subtractions in a row
  combine         the same with k terms;  apply_interior: (row length + 1) 2^-52 * sum_j |a_rj x_j|

Sizes: n = 1 (a lone tail row), 63 / 64 / 65 and 255 / 257 (odd, around a wave and half a workgroup's rows), 4099
(several workgroups) and 525319: past the 1024 x 512 rows one trip of the capped grid covers, odd.  j = 0, 1, 7, 29:
one, one, one and four register blocks of eight columns.  Entries have mixed magnitudes (2^-20 .. 2^20)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [1, 63, 64, 65, 255, 257, 4099, 1024 * 512 + 1031]
JS = [0, 1, 7, 29]
RESTART = 30
U = 2.0 ** -53
LD = np.longdouble

_data, _objs = {}, {}


def data(n):
    """(V: 31 columns, w, h: 30 coefficients) for size n: computed once, never written to."""
    if n not in _data:
        rng = np.random.default_rng(1000 + n % 997)
        V = rng.standard_normal((RESTART + 1, n)) * 2.0 ** rng.integers(-20, 21, size=(RESTART + 1, n))
        w = rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, size=n)
        h = rng.standard_normal(RESTART) * 2.0 ** rng.integers(-8, 9, size=RESTART)
        for a in (V, w, h):
            a.setflags(write=False)
        _data[n] = (V, w, h)
    return _data[n]


def put(schwz, torch, host, ptr):
    t = torch.from_numpy(np.array(host, dtype=np.float64)).cuda()  # (a copy: the shared inputs are read-only)
    schwz.outer_copy(len(host), t.data_ptr(), ptr)
    torch.cuda.synchronize()


def get(schwz, torch, ptr, n):
    t = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    schwz.outer_copy(n, ptr, t.data_ptr())
    torch.cuda.synchronize()
    return t.cpu().numpy()[:n]


def outer_with_basis(schwz, torch, n):
    """One schwz_outer per size with V_0 .. V_29 uploaded (the tests rewrite w and V_30 only)."""
    if n not in _objs:
        V, _, _ = data(n)
        o = schwz.Outer(n, RESTART)
        for i in range(RESTART):
            put(schwz, torch, V[i], o.vector(o.V, i))
        _objs[n] = o
    return _objs[n]


def gamma(n):
    return n * U / (1.0 - n * U)


def check_dots(got, V, w, j, n):
    """got = [V_0 . w, ..., V_j . w, w . w] of the device against longdouble, at the bound of a dot of length n."""
    wl = w.astype(LD)
    for i in range(j + 2):
        v = wl if i == j + 1 else V[i].astype(LD)
        ref, mag = np.sum(v * wl), float(np.sum(np.abs(v * wl)))
        assert abs(float(LD(got[i]) - ref)) <= gamma(n) * mag, (n, j, i, got[i], float(ref))


@pytest.mark.parametrize("j", JS)
@pytest.mark.parametrize("n", SIZES)
def test_dots(schwz, torch_cuda, n, j):
    V, w, _ = data(n)
    o = outer_with_basis(schwz, torch_cuda, n)
    put(schwz, torch_cuda, w, o.vector(o.W))
    got = o.dots(j)
    assert got.shape == (j + 2,)
    check_dots(got, V, w, j, n)
    again = o.dots(j)
    assert got.tobytes() == again.tobytes()  # fixed order of every sum: the same bits
    assert get(schwz, torch_cuda, o.vector(o.W), n).tobytes() == w.tobytes()  # w is only read


@pytest.mark.parametrize("j", JS)
@pytest.mark.parametrize("n", SIZES)
def test_project_dots(schwz, torch_cuda, n, j):
    V, w, h = data(n)
    o = outer_with_basis(schwz, torch_cuda, n)
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


@pytest.mark.parametrize("n", SIZES)
def test_start_and_normalize_scale_w_exactly(schwz, torch_cuda, n):
    """One multiplication per entry: the bits of numpy's product.  V_30 and V_0 are written, V_0 is put back."""
    V, w, _ = data(n)
    o = outer_with_basis(schwz, torch_cuda, n)
    put(schwz, torch_cuda, w, o.vector(o.W))
    o.normalize(RESTART - 1, 0.3)
    assert get(schwz, torch_cuda, o.vector(o.V, RESTART), n).tobytes() == (w * 0.3).tobytes()
    o.start(1.0 / 7.0)
    assert get(schwz, torch_cuda, o.vector(o.V, 0), n).tobytes() == (w * (1.0 / 7.0)).tobytes()
    assert get(schwz, torch_cuda, o.vector(o.V, 1), n).tobytes() == V[1].tobytes()  # the neighbouring column is intact
    put(schwz, torch_cuda, V[0], o.vector(o.V, 0))


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [1, 65, 4099, 1024 * 512 + 1031])
def test_copy_at_any_alignment(schwz, torch_cuda, n, shift):
    torch = torch_cuda
    src = torch.arange(n + 2, dtype=torch.float64, device="cuda") * 0.5
    dst = torch.full((n + 3,), -1.0, dtype=torch.float64, device="cuda")
    schwz.outer_copy(n, src.data_ptr() + 8 * shift, dst.data_ptr() + 8)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert host[0] == -1.0 and (host[n + 1:] == -1.0).all()
    assert np.array_equal(host[1:n + 1], (np.arange(n + 2) * 0.5)[shift:shift + n])


# ---- lap3d_16x10x7 on three subdomains: combine and the operator ------------------------------------------------------

LAP = (16, 10, 7)
N = 16 * 10 * 7
FR3 = np.array([0, 30, 575, N], dtype=np.int64)


@pytest.fixture(scope="module")
def lap_solver(schwz):
    part = np.searchsorted(FR3, np.arange(N), side="right") - 1
    s = schwz.Settings(laplacian_dim=3, laplacian_shape=LAP, partition=schwz.PARTITION_CUSTOM, partition_vector=part)
    m = schwz.Metadata(num_subdomains=3, tolerance=1e-8, max_iters=50, local_precond="block-jacobi",
                       precond_max_block_size=1, local_solver_tolerance=0.0, local_max_iters=10)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(3), quiet=True)
    solver.initialize()
    assert list(m.first_row) == list(FR3) and (m.permutation is None or np.array_equal(m.permutation, np.arange(N)))
    return solver


@pytest.mark.parametrize("k", [1, 7, 30])
@pytest.mark.parametrize("shift", [0, 1])
def test_combine_against_numpy(schwz, torch_cuda, k, shift):
    """x += sum_{i<k} y_i Z_i over the 1120 rows, x 16-byte aligned and not."""
    torch = torch_cuda
    rng = np.random.default_rng(5 + k)
    Z = rng.standard_normal((k, N)) * 2.0 ** rng.integers(-20, 21, size=(k, N))
    y = rng.standard_normal(k) * 2.0 ** rng.integers(-8, 9, size=k)
    x0 = rng.standard_normal(N)
    o = schwz.Outer(N, RESTART)
    for i in range(k):
        put(schwz, torch, Z[i], o.vector(o.Z, i))
    x = torch.zeros(N + 2, dtype=torch.float64, device="cuda")
    x[shift:shift + N] = torch.from_numpy(x0).cuda()
    o.combine(y, x.data_ptr() + 8 * shift)
    torch.cuda.synchronize()
    host = x.cpu().numpy()
    terms = y[:, None].astype(LD) * Z.astype(LD)
    ref = x0.astype(LD) + terms.sum(axis=0)
    bound = (k + 2) * 2.0 ** -52 * (np.abs(x0) + np.abs(terms).sum(axis=0).astype(np.float64))
    assert (np.abs((host[shift:shift + N].astype(LD) - ref).astype(np.float64)) <= bound).all()
    assert (host[:shift] == 0.0).all() and (host[shift + N:] == 0.0).all()


def test_apply_interior_against_numpy(schwz, oracle, torch_cuda, lap_solver):
    """x into the interiors of x~, one exchange, (A x~) on the interior rows of the three subdomains side by side in
    one vector -- offsets 0, 30 and 575, the last one odd -- against the rows of the global matrix."""
    import scipy.sparse as sp
    from schwz_amd import outer
    torch, solver = torch_cuda, lap_solver
    rp, col, val = oracle.laplacian3d(*LAP)
    A = sp.csr_matrix((val, col, rp), shape=(N, N))
    x = np.random.default_rng(11).standard_normal(N) * 2.0 ** np.random.default_rng(12).integers(-10, 11, size=N)
    xd = torch.from_numpy(x).cuda()
    out = torch.full((N + 1,), -7.0, dtype=torch.float64, device="cuda")
    stream = solver.backend.stream()
    for me, sd in solver.subdomains.items():
        assert sd.local_size == FR3[me + 1] - FR3[me]
        schwz.outer_copy(sd.local_size, xd.data_ptr() + 8 * int(FR3[me]), sd.vector(0)[0], stream)
    outer._exchange(solver, stream)
    for me, sd in solver.subdomains.items():
        sd.apply_interior(out.data_ptr() + 8 * int(FR3[me]), stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    absA = sp.csr_matrix((np.abs(val), col, rp), shape=(N, N))
    ref = np.array([np.sum(val[rp[r]:rp[r + 1]].astype(LD) * x[col[rp[r]:rp[r + 1]]].astype(LD)) for r in range(N)])
    bound = (np.diff(rp) + 1) * 2.0 ** -52 * (absA @ np.abs(x))
    assert (np.abs((host[:N].astype(LD) - ref).astype(np.float64)) <= bound).all()
    assert host[N] == -7.0
    assert np.allclose(host[:N], A @ x, rtol=0, atol=1e-9 * np.abs(x).max())
    # the subdomains are left as a fresh set_rhs leaves them
    solver.set_rhs(None, "zero")
