"""A destroyed object gives its device memory back: schwz_csr, schwz_trs (level plan with its graph cache and capture
stream; Jacobi sweeps) and an uploaded schwz_subdomain.

Every one of them owns its HIP resources through self-freeing members, and its destroy function is `delete`.  The
check is by free-memory readings (torch.cuda.mem_get_info): after a warm-up cycle, the footprint F of one live object
is measured, then the object is created, used and closed 8 more times, and free memory must not have fallen by more
than F / 2.  That catches an object that leaks a sixteenth of itself or more per cycle.

What this cannot show: the runtime hands out device memory in coarse granules, so a buffer far below F / 16 -- a
forgotten 4-byte flag, say -- is invisible to free-memory readings.  That no raw allocation is left in the sources is
what guards those (hipMalloc / hipFree and their kin appear only inside the owning types of csrc/schwz_internal.hpp and
in the C ABI's own allocate / free pairs).  The shapes are chosen so that F is at least 16 MiB, below which the
granularity could hide a whole buffer; the floor is asserted, so a shape that is too small fails instead of passing
emptily."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

NX = 512                 # 512 x 512 five-point matrix: 262144 rows, 1.3 M entries
F_MIN = 16 << 20
CYCLES = 8


def _five_point(nx):
    t = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx), format="csr")
    eye = sp.identity(nx, format="csr")
    a = (sp.kron(eye, t) + sp.kron(t, eye)).tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


@pytest.fixture(scope="module")
def five_point():
    return _five_point(NX)


@pytest.fixture(scope="module")
def ilu_factors(schwz, five_point):
    f = schwz.ilu0(*five_point)
    return tuple(f[k] for k in ("l_rp", "l_col", "l_val", "u_rp", "u_col", "u_val"))


def _free(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _gives_memory_back(torch, cycle, tag):
    """cycle(keep) creates the object, uses it and, unless keep, closes it; it returns the object."""
    cycle(False)                                     # warm-up: code objects, the runtime's own pools
    before = _free(torch)
    obj = cycle(True)
    footprint = before - _free(torch)
    obj.close()
    for _ in range(CYCLES):
        cycle(False)
    lost = before - _free(torch)
    print("%s: footprint %.1f MiB, free memory fell by %.2f MiB over %d cycles" %
          (tag, footprint / 2.0 ** 20, lost / 2.0 ** 20, CYCLES + 1))
    assert footprint >= F_MIN, "%s: footprint %d B is below the %d B at which a leak can be seen" % (tag, footprint, F_MIN)
    assert lost <= footprint // 2, "%s: %d B of %d B not given back" % (tag, lost, footprint)


def test_csr_gives_its_memory_back(schwz, torch_cuda, five_point):
    torch = torch_cuda
    n = len(five_point[0]) - 1
    x = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")

    def cycle(keep):
        a = schwz.Csr(*five_point)
        a.spmv(x.data_ptr(), y.data_ptr())
        if not keep:
            a.close()
        return a

    _gives_memory_back(torch, cycle, "Csr")


def test_trs_level_plan_gives_its_memory_back(schwz, torch_cuda, ilu_factors, monkeypatch):
    """SCHWZ_TRS_FLAGS=0 at creation: the level-by-level plan, whose first solve creates the capture stream and
    records a graph (SCHWZ_TRS_GRAPH left at its default), and whose second solve with the same pointers replays it."""
    torch = torch_cuda
    n = len(ilu_factors[0]) - 1
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    monkeypatch.setenv("SCHWZ_TRS_FLAGS", "0")
    monkeypatch.delenv("SCHWZ_TRS_GRAPH", raising=False)

    def cycle(keep):
        t = schwz.Trs(*ilu_factors)
        t.solve(b.data_ptr(), y.data_ptr())          # records the graph
        t.solve(b.data_ptr(), y.data_ptr())          # replays it
        if not keep:
            torch.cuda.synchronize()
            t.close()
        return t

    _gives_memory_back(torch, cycle, "Trs, level plan")


def test_trs_sweeps_gives_its_memory_back(schwz, torch_cuda, ilu_factors):
    torch = torch_cuda
    n = len(ilu_factors[0]) - 1
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")

    def cycle(keep):
        t = schwz.TrsSweeps(*ilu_factors, 2)
        t.solve(b.data_ptr(), y.data_ptr())
        if not keep:
            torch.cuda.synchronize()
            t.close()
        return t

    _gives_memory_back(torch, cycle, "TrsSweeps")


def test_uploaded_subdomain_gives_its_memory_back(schwz, torch_cuda):
    """The first half of the 720 x 720 five-point problem with overlap 2 (interface rows, get lists, halo), uploaded
    with CG + Jacobi; one local solve, one restriction and one rhs_gather, so that the second x~ buffer and the
    device copy of the index map exist."""
    torch = torch_cuda
    prob = schwz.Problem.laplacian(2, 720)
    N = 720 * 720
    fr = np.array([0, N // 2, N], dtype=np.int64)
    g = torch.ones(N, dtype=torch.float64, device="cuda")

    def cycle(keep):
        sd = schwz.Subdomain(prob, 2, 0, 2, fr)
        sd.to_device(np.ones(sd.local_size_x), precond=schwz.capi.PRECOND_JACOBI, local_tol=0.0, local_max_iters=4)
        sd.local_solve()
        sd.restrict()
        sd.rhs_gather(g.data_ptr(), N)
        if not keep:
            torch.cuda.synchronize()
            sd.close()
        return sd

    _gives_memory_back(torch, cycle, "Subdomain")
    prob.close()
