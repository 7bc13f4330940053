"""Thin object wrappers over the C ABI (include/schwz_hip.h).

Device buffers are plain integer addresses here (torch supplies them in the
host layer: `tensor.data_ptr()`); host arrays are numpy.
"""
import ctypes as C

import numpy as np

from . import _capi as capi
from ._capi import check, lib, ptr

IDX = np.int32


def _stream_arg(stream):
    return C.c_void_p(int(stream)) if stream else None


# ---------------------------------------------------------------------------
# stand-alone device objects
# ---------------------------------------------------------------------------

def gather(n, d_idx, d_from, d_into, op=capi.OP_COPY, stream=0):
    """gather_kernel.cu:46-109."""
    check(lib.schwz_gather(n, ptr(d_idx), ptr(d_from), ptr(d_into), op, _stream_arg(stream)))


def scatter(n, d_idx, d_from, d_into, op=capi.OP_COPY, stream=0):
    """scatter_kernel.cu:43-107."""
    check(lib.schwz_scatter(n, ptr(d_idx), ptr(d_from), ptr(d_into), op, _stream_arg(stream)))


class Csr:
    """A CSR matrix resident in HBM (gko::matrix::Csr on the device executor)."""

    def __init__(self, rp, col, val, ncols=None):
        rp = np.ascontiguousarray(rp, dtype=IDX)
        col = np.ascontiguousarray(col, dtype=IDX)
        val = np.ascontiguousarray(val, dtype=np.float64)
        self.nrows = len(rp) - 1
        self.ncols = self.nrows if ncols is None else ncols
        h = C.c_void_p()
        check(lib.schwz_csr_create(self.nrows, self.ncols, ptr(rp), ptr(col), ptr(val), C.byref(h)))
        self.h = h
        self.nnz = int(lib.schwz_csr_nnz(h))

    def spmv(self, d_x, d_y, alpha=1.0, beta=0.0, variant=0, stream=0):
        check(lib.schwz_csr_spmv(self.h, alpha, ptr(d_x), beta, ptr(d_y), variant,
                                 _stream_arg(stream)))

    def spmm(self, d_x, d_y, k, alpha=1.0, beta=0.0, stream=0):
        """Y = alpha A X + beta Y on block vectors of k = 2, 4 or 8 columns, element (i, j) at i * k + j
        (schwz_csr_spmm, an extension); plain CSR whatever format() says."""
        check(lib.schwz_csr_spmm(self.h, int(k), alpha, ptr(d_x), beta, ptr(d_y), _stream_arg(stream)))

    def format(self):
        """Coding variant 0 uses: 0 plain CSR, 1 per-entry dictionaries, 2 row patterns, 3 row pairs."""
        return int(lib.schwz_csr_format(self.h))

    def symmetric(self):
        """True when the upload found the (row-pair coded) matrix symmetric bit for bit."""
        return bool(lib.schwz_csr_symmetric(self.h))

    def sweep_slots(self):
        """Workgroup slots of the z-sweep walk of the CG update launch (0: not a canonical 3-D stencil)."""
        return int(lib.schwz_csr_sweep_slots(self.h))

    def sweep_left_out(self):
        """Chunks of 512 rows the z-sweep walk leaves to its companion launch."""
        return int(lib.schwz_csr_sweep_left_out(self.h))

    def algorithmic_bytes(self):
        # 12 nnz + 4 (rows+1) + 16 rows
        return 12 * self.nnz + 4 * (self.nrows + 1) + 16 * self.nrows

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_csr_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Pcg:
    """Device-resident preconditioned CG (gko::solver::Cg + stop::Combined)."""

    def __init__(self, csr, precond=capi.PRECOND_NONE, block_size=1, par_ilu_sweeps=0, trisolve_sweeps=0):
        self.csr = csr
        h = C.c_void_p()
        if par_ilu_sweeps or trisolve_sweeps:
            # ilu / isai with ParILU factors and / or Jacobi-sweep solves (schwz_pcg_create_ilu)
            check(lib.schwz_pcg_create_ilu(csr.h, precond, int(par_ilu_sweeps), int(trisolve_sweeps), C.byref(h)))
        else:
            check(lib.schwz_pcg_create_ex(csr.h, precond, block_size, C.byref(h)))
        self.h = h

    def solve(self, d_b, d_x, rtol, max_iters, stream=0, want_stats=True):
        it = C.c_int(0)
        rn = C.c_double(0.0)
        check(lib.schwz_pcg_solve(self.h, ptr(d_b), ptr(d_x), rtol, max_iters,
                                  C.byref(it) if want_stats else None,
                                  C.byref(rn) if want_stats else None, _stream_arg(stream)))
        return it.value, rn.value

    def flavour(self):
        """How the last solve iterated (schwz_pcg_flavour)."""
        return int(lib.schwz_pcg_flavour(self.h))

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_pcg_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class PcgF32:
    """Mixed-precision CG (schwz_pcg_f32): fp32 PCG on the fp64 start residual, the correction added in fp64.
    precond: PRECOND_NONE or PRECOND_JACOBI."""

    def __init__(self, csr, precond=capi.PRECOND_NONE):
        self.csr = csr
        h = C.c_void_p()
        check(lib.schwz_pcg_f32_create(csr.h, precond, C.byref(h)))
        self.h = h

    def solve(self, d_b, d_x, rtol, max_iters, stream=0, want_stats=True):
        it = C.c_int(0)
        rn = C.c_double(0.0)
        check(lib.schwz_pcg_f32_solve(self.h, ptr(d_b), ptr(d_x), rtol, max_iters,
                                      C.byref(it) if want_stats else None,
                                      C.byref(rn) if want_stats else None, _stream_arg(stream)))
        return it.value, rn.value

    def spmv(self, d_p, d_q, stream=0):
        """q = A32 p by the launch of the iteration (fp32 device vectors); returns p.q as that launch sums it."""
        pq = C.c_double(0.0)
        check(lib.schwz_pcg_f32_spmv(self.h, ptr(d_p), ptr(d_q), C.byref(pq), _stream_arg(stream)))
        return pq.value

    def last_stats(self):
        it, rn = C.c_int(0), C.c_double(0.0)
        check(lib.schwz_pcg_f32_last_stats(self.h, C.byref(it), C.byref(rn)))
        return it.value, rn.value

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_pcg_f32_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Bicgstab:
    """Device-resident BiCGSTAB, right preconditioned (schwz_bicgstab, an extension: the reference's non-symmetric
    local solver is GMRES).  solve() returns (iterations, recurred residual norm); breakdown() the flag of the last
    solve: 0 none, 1 rho = 0, 2 rhat.v = 0, 3 t.t = 0 or t.s = 0."""

    def __init__(self, csr, precond=capi.PRECOND_NONE, block_size=1, par_ilu_sweeps=0, trisolve_sweeps=0):
        self.csr = csr
        h = C.c_void_p()
        check(lib.schwz_bicgstab_create(csr.h, precond, block_size, int(par_ilu_sweeps), int(trisolve_sweeps),
                                        C.byref(h)))
        self.h = h

    def solve(self, d_b, d_x, rtol, max_iters, stream=0, want_stats=True):
        it = C.c_int(0)
        rn = C.c_double(0.0)
        check(lib.schwz_bicgstab_solve(self.h, ptr(d_b), ptr(d_x), rtol, max_iters,
                                       C.byref(it) if want_stats else None,
                                       C.byref(rn) if want_stats else None, _stream_arg(stream)))
        return it.value, rn.value

    def last_stats(self):
        it, rn = C.c_int(0), C.c_double(0.0)
        check(lib.schwz_bicgstab_last_stats(self.h, C.byref(it), C.byref(rn)))
        return it.value, rn.value

    def breakdown(self):
        flag = int(lib.schwz_bicgstab_breakdown(self.h))
        if flag < 0:   # the device state could not be read
            check(capi.ERR_HIP)
        return flag

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_bicgstab_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Chebyshev:
    """Device-resident Chebyshev iteration for SPD matrices, one reduction-free launch per iteration (schwz_cheb, an
    extension: the reference's symmetric local solver is CG).  precond: PRECOND_NONE or PRECOND_JACOBI.  The bounds
    on the spectrum of M^-1 A start as (Gershgorin bound / 30, Gershgorin bound); better ones are the caller's
    (set_bounds), and an upper bound below the true one makes the iteration diverge.  solve() returns (corrections
    applied, recurred residual norm); with rtol <= 0 the norm costs one more matrix pass and is computed only when
    asked for."""

    def __init__(self, csr, precond=capi.PRECOND_NONE):
        self.csr = csr
        h = C.c_void_p()
        check(lib.schwz_cheb_create(csr.h, precond, C.byref(h)))
        self.h = h

    def bounds(self):
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        check(lib.schwz_cheb_bounds(self.h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def set_bounds(self, lmin, lmax):
        check(lib.schwz_cheb_set_bounds(self.h, float(lmin), float(lmax)))

    def solve(self, d_b, d_x, rtol, max_iters, stream=0, want_stats=True):
        it = C.c_int(0)
        rn = C.c_double(0.0)
        check(lib.schwz_cheb_solve(self.h, ptr(d_b), ptr(d_x), rtol, max_iters,
                                   C.byref(it) if want_stats else None,
                                   C.byref(rn) if want_stats else None, _stream_arg(stream)))
        return it.value, rn.value

    def last_stats(self):
        it, rn = C.c_int(0), C.c_double(0.0)
        check(lib.schwz_cheb_last_stats(self.h, C.byref(it), C.byref(rn)))
        return it.value, rn.value

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_cheb_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class BatchCg:
    """k = 2, 4 or 8 independent CG recurrences that share one pass over the matrix per iteration (schwz_bcg, an
    extension: the reference solves one system).  precond: PRECOND_NONE or PRECOND_JACOBI.  Block vectors are
    row-interleaved, element (i, j) at i * k + j.  solve() returns per-column lists (updates applied, recurred residual
    norm); a column is frozen -- its x stops changing -- once its own test fires, where it would divide by zero, or
    from the start where bit j of `frozen` is set."""

    def __init__(self, csr, precond=capi.PRECOND_NONE, k=8):
        self.csr, self.k = csr, int(k)
        h = C.c_void_p()
        check(lib.schwz_bcg_create(csr.h, precond, self.k, C.byref(h)))
        self.h = h

    def solve(self, d_b, d_x, rtol, max_iters, frozen=0, stream=0, want_stats=True):
        it = (C.c_int * self.k)()
        rn = (C.c_double * self.k)()
        check(lib.schwz_bcg_solve(self.h, ptr(d_b), ptr(d_x), rtol, max_iters, int(frozen),
                                  it if want_stats else None, rn if want_stats else None, _stream_arg(stream)))
        return list(it), list(rn)

    def last_stats(self):
        it = (C.c_int * self.k)()
        rn = (C.c_double * self.k)()
        check(lib.schwz_bcg_last_stats(self.h, it, rn))
        return list(it), list(rn)

    def residual(self, d_b, d_x, d_r=None, stream=0):
        """Per column ||b_j - A x_j||^2 (waits for the stream); R = B - A X goes to d_r where one is given."""
        out = (C.c_double * self.k)()
        check(lib.schwz_bcg_residual(self.h, ptr(d_b), ptr(d_x), ptr(d_r), out, _stream_arg(stream)))
        return list(out)

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_bcg_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Gmres:
    """Device-resident restarted GMRES, right preconditioned (gko::solver::Gmres with
    krylov_dim = restart; solve.cpp:486-520)."""

    def __init__(self, csr, precond=capi.PRECOND_NONE, block_size=1, restart=1, par_ilu_sweeps=0,
                 trisolve_sweeps=0, basis=capi.GMRES_BASIS_F64):
        """basis: capi.GMRES_BASIS_F64, or capi.GMRES_BASIS_F32 for the compressed basis (fp32 Krylov vectors, fp64
        arithmetic, blocked CGS2: schwz_gmres_create_basis)."""
        self.csr = csr
        h = C.c_void_p()
        if basis != capi.GMRES_BASIS_F64:
            check(lib.schwz_gmres_create_basis(csr.h, precond, block_size, restart, int(par_ilu_sweeps),
                                               int(trisolve_sweeps), int(basis), C.byref(h)))
        elif par_ilu_sweeps or trisolve_sweeps:
            check(lib.schwz_gmres_create_ex(csr.h, precond, block_size, restart, int(par_ilu_sweeps),
                                            int(trisolve_sweeps), C.byref(h)))
        else:
            check(lib.schwz_gmres_create(csr.h, precond, block_size, restart, C.byref(h)))
        self.h = h

    def solve(self, d_b, d_x, rtol, max_iters, stream=0, want_stats=True):
        it = C.c_int(0)
        rn = C.c_double(0.0)
        check(lib.schwz_gmres_solve(self.h, ptr(d_b), ptr(d_x), rtol, max_iters,
                                    C.byref(it) if want_stats else None,
                                    C.byref(rn) if want_stats else None, _stream_arg(stream)))
        return it.value, rn.value

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_gmres_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Trs:
    """y = P^T L^-T L^-1 P b (gko LowerTrs/UpperTrs + Permutation)."""

    def __init__(self, l_rp, l_col, l_val, u_rp, u_col, u_val, perm=None):
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
                ((l_rp, IDX), (l_col, IDX), (l_val, np.float64), (u_rp, IDX), (u_col, IDX),
                 (u_val, np.float64))]
        arrs.append(None if perm is None else np.ascontiguousarray(perm, dtype=IDX))
        self.n = len(l_rp) - 1
        h = C.c_void_p()
        check(lib.schwz_trs_create(self.n, *[ptr(a) for a in arrs], C.byref(h)))
        self.h = h

    def solve(self, d_b, d_y, stream=0):
        check(lib.schwz_trs_solve(self.h, ptr(d_b), ptr(d_y), _stream_arg(stream)))

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_trs_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class TrsLU(Trs):
    """y = Q U^-1 L^-1 P b for A(row_perm, col_perm) = L U (schwz_lu factors)."""

    def __init__(self, l_rp, l_col, l_val, u_rp, u_col, u_val, row_perm, col_perm):
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
                ((l_rp, IDX), (l_col, IDX), (l_val, np.float64), (u_rp, IDX), (u_col, IDX),
                 (u_val, np.float64), (row_perm, IDX), (col_perm, IDX))]
        self.n = len(l_rp) - 1
        h = C.c_void_p()
        check(lib.schwz_trs_create_lu(self.n, *[ptr(a) for a in arrs], C.byref(h)))
        self.h = h


class TrsSweeps(Trs):
    """y = U^-1 L^-1 b with each factor applied by `sweeps` Jacobi passes: x_0 = D^-1 b,
    x_{m+1} = D^-1 (b - T_s x_m) (schwz_trs_create_sweeps)."""

    def __init__(self, l_rp, l_col, l_val, u_rp, u_col, u_val, sweeps):
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
                ((l_rp, IDX), (l_col, IDX), (l_val, np.float64), (u_rp, IDX), (u_col, IDX),
                 (u_val, np.float64))]
        self.n = len(l_rp) - 1
        h = C.c_void_p()
        check(lib.schwz_trs_create_sweeps(self.n, *[ptr(a) for a in arrs], int(sweeps), C.byref(h)))
        self.h = h

    @property
    def sweeps(self):
        return int(lib.schwz_trs_sweeps(self.h))


def ilu0(rp, col, val):
    """Host ILU(0) standing in for gko::factorization::ParIlu (solve.cpp:506-532)."""
    return _ilu_factors(lib.schwz_ilu0, rp, col, val)


def parilu(rp, col, val, sweeps):
    """ILU(0)-pattern factors from `sweeps` synchronous ParILU sweeps on the GPU
    (gko::factorization::ParIlu, solve.cpp:506-532); same layout as ilu0."""
    return _ilu_factors(lambda n, *a: lib.schwz_parilu_host(n, *a[:3], int(sweeps), *a[3:]), rp, col, val)


def _ilu_factors(fn, rp, col, val):
    rp = np.ascontiguousarray(rp, dtype=IDX)
    col = np.ascontiguousarray(col, dtype=IDX)
    val = np.ascontiguousarray(val, dtype=np.float64)
    n = len(rp) - 1
    out = [C.c_void_p() for _ in range(6)]
    check(fn(n, ptr(rp), ptr(col), ptr(val), *[C.byref(o) for o in out]))

    def take(p, cnt, ctype, dtype):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(max(cnt, 1),))[:cnt].copy().astype(dtype)

    l_rp = take(out[0], n + 1, C.c_int32, IDX)
    u_rp = take(out[3], n + 1, C.c_int32, IDX)
    res = dict(l_rp=l_rp, l_col=take(out[1], int(l_rp[-1]), C.c_int32, IDX),
               l_val=take(out[2], int(l_rp[-1]), C.c_double, np.float64), u_rp=u_rp,
               u_col=take(out[4], int(u_rp[-1]), C.c_int32, IDX),
               u_val=take(out[5], int(u_rp[-1]), C.c_double, np.float64))
    for o in out:
        lib.schwz_free(o)
    return res


def isai(rp, col, val, lower):
    """ISAI values of a triangular CSR factor on its own pattern (LowerIsai / UpperIsai,
    solve.cpp:616-638)."""
    rp = np.ascontiguousarray(rp, dtype=IDX)
    col = np.ascontiguousarray(col, dtype=IDX)
    val = np.ascontiguousarray(val, dtype=np.float64)
    n = len(rp) - 1
    out = C.c_void_p()
    check(lib.schwz_isai(n, ptr(rp), ptr(col), ptr(val), int(bool(lower)), C.byref(out)))
    nnz = int(rp[-1])
    w = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_double)), shape=(max(nnz, 1),))[:nnz].copy()
    lib.schwz_free(out)
    return w


def cholesky(rp, col, val, natural=False):
    """Host sparse LL^T standing in for CHOLMOD (solve.cpp:75-143)."""
    rp = np.ascontiguousarray(rp, dtype=IDX)
    col = np.ascontiguousarray(col, dtype=IDX)
    val = np.ascontiguousarray(val, dtype=np.float64)
    n = len(rp) - 1
    out = [C.c_void_p() for _ in range(7)]
    check(lib.schwz_cholesky(n, ptr(rp), ptr(col), ptr(val), int(natural),
                             *[C.byref(o) for o in out]))

    def take(p, cnt, ctype, dtype):
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(max(cnt, 1),))[:cnt].copy()
        return a.astype(dtype, copy=False)

    l_rp = take(out[0], n + 1, C.c_int32, IDX)
    lnz = int(l_rp[-1]) if n else 0
    res = dict(l_rp=l_rp, l_col=take(out[1], lnz, C.c_int32, IDX),
               l_val=take(out[2], lnz, C.c_double, np.float64),
               u_rp=take(out[3], n + 1, C.c_int32, IDX),
               u_col=take(out[4], lnz, C.c_int32, IDX),
               u_val=take(out[5], lnz, C.c_double, np.float64),
               perm=take(out[6], n, C.c_int32, IDX))
    for o in out:
        lib.schwz_free(o)
    return res


class DeviceWindow:
    """A device buffer other rank processes of the node can map (MPI_Win_create of
    communicate.hpp:67-224 over HIP IPC).  `handle` travels to the peers over any host channel."""

    def __init__(self, count, single=False):
        self.count, self.esize = int(count), 4 if single else 8
        p = C.c_void_p()
        check(lib.schwz_window_alloc(self.count * self.esize, C.byref(p)))
        self.ptr = p.value
        buf = (C.c_ubyte * 64)()
        check(lib.schwz_window_export(C.c_void_p(self.ptr), buf))
        self.handle = ("hip-ipc", bytes(buf), self.count, self.esize)

    def at(self, offset):
        return self.ptr + int(offset) * self.esize

    def close(self):
        if getattr(self, "ptr", None) and lib is not None:
            lib.schwz_window_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        self.close()


class PeerWindow:
    """Another rank's DeviceWindow mapped into this process."""

    def __init__(self, handle):
        kind, raw, self.count, self.esize = handle
        assert kind == "hip-ipc"
        buf = (C.c_ubyte * 64).from_buffer_copy(raw)
        p = C.c_void_p()
        check(lib.schwz_window_open(buf, C.byref(p)))
        self.ptr = p.value

    def at(self, offset):
        return self.ptr + int(offset) * self.esize

    def close(self):
        if getattr(self, "ptr", None) and lib is not None:
            lib.schwz_window_close(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        self.close()


def host_atomic_add(arr, index, v=1):
    """MPI_Accumulate(MPI_SUM) on an int32 of a shared-memory window."""
    return int(lib.schwz_host_atomic_add_i32(C.c_void_p(arr.ctypes.data + 4 * int(index)), int(v)))


def host_atomic_min(arr, index, v):
    """MPI_Accumulate(MPI_MIN) on a float64 of a shared-memory window."""
    return float(lib.schwz_host_atomic_min_f64(C.c_void_p(arr.ctypes.data + 8 * int(index)), float(v)))


# ---------------------------------------------------------------------------
# host setup
# ---------------------------------------------------------------------------

class Problem:
    """Global system matrix as a row source (never replicated per rank)."""

    def __init__(self, handle):
        self.h = handle
        self.N = int(lib.schwz_problem_size(handle))
        self.nnz = int(lib.schwz_problem_nnz(handle))

    @classmethod
    def laplacian(cls, dim, nx, ny=None, nz=None):
        """initialization.cpp:214-265 (dim=2) and its 3-D 7-point extension."""
        ny = nx if ny is None else ny
        nz = (1 if dim == 2 else nx) if nz is None else nz
        h = C.c_void_p()
        check(lib.schwz_problem_laplacian(dim, nx, ny, nz, C.byref(h)))
        return cls(h)

    @staticmethod
    def _check_lengths(who, rp, col, val):
        """The library reads col and val up to row_ptr[-1]: arrays that end before that are refused here."""
        if rp.ndim != 1 or col.ndim != 1 or val.ndim != 1 or len(rp) < 1:
            raise capi.SchwzError(capi.ERR_INVALID, who + ": row_ptr, col and val must be 1-D, row_ptr not empty")
        if min(len(col), len(val)) < int(rp[-1]):
            raise capi.SchwzError(capi.ERR_INVALID, "%s: row_ptr ends at %d, col holds %d and val %d entries"
                             % (who, int(rp[-1]), len(col), len(val)))

    @classmethod
    def from_csr(cls, rp, col, val):
        """Rows may be unsorted and may hold a column more than once: they are stable-sorted and the entries of one
        column summed in stored order (schwz_problem_from_csr)."""
        rp = np.ascontiguousarray(rp, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=IDX)
        val = np.ascontiguousarray(val, dtype=np.float64)
        cls._check_lengths("Problem.from_csr", rp, col, val)
        h = C.c_void_p()
        check(lib.schwz_problem_from_csr(len(rp) - 1, ptr(rp), ptr(col), ptr(val), C.byref(h)))
        return cls(h)

    @classmethod
    def from_rows(cls, N, row_ids, rp, col, val):
        """A row source that holds the rows `row_ids` (ascending global ids) of an N x N matrix only:
        what a rank receives in the distributed ingest (schwz_problem_from_rows)."""
        row_ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        rp = np.ascontiguousarray(rp, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=IDX)
        val = np.ascontiguousarray(val, dtype=np.float64)
        cls._check_lengths("Problem.from_rows", rp, col, val)
        if row_ids.ndim != 1 or len(rp) != len(row_ids) + 1:
            raise capi.SchwzError(capi.ERR_INVALID, "Problem.from_rows: row_ptr must hold len(row_ids) + 1 entries")
        h = C.c_void_p()
        check(lib.schwz_problem_from_rows(int(N), len(row_ids), ptr(row_ids), ptr(rp), ptr(col), ptr(val),
                                          C.byref(h)))
        return cls(h)

    def extract_rows(self, row_ids):
        """(rp, col, val) of the rows `row_ids`, columns global (schwz_problem_extract_rows)."""
        row_ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        rp = np.zeros(len(row_ids) + 1, dtype=np.int64)
        check(lib.schwz_problem_extract_rows(self.h, len(row_ids), ptr(row_ids), ptr(rp), None, None))
        col = np.zeros(max(int(rp[-1]), 1), dtype=IDX)
        val = np.zeros(max(int(rp[-1]), 1), dtype=np.float64)
        check(lib.schwz_problem_extract_rows(self.h, len(row_ids), ptr(row_ids), ptr(rp), ptr(col), ptr(val)))
        return rp, col[:rp[-1]], val[:rp[-1]]

    @classmethod
    def from_matrix_market(cls, path):
        """initialization.cpp:204-213."""
        h = C.c_void_p()
        check(lib.schwz_problem_from_matrix_market(path.encode(), C.byref(h)))
        return cls(h)

    def row(self, g):
        cap = 64
        while True:
            cols = np.zeros(cap, dtype=np.int64)
            vals = np.zeros(cap, dtype=np.float64)
            n = C.c_int(0)
            rc = lib.schwz_problem_row(self.h, g, C.byref(n), ptr(cols), ptr(vals), cap)
            if rc == capi.ERR_INVALID and cap < (1 << 24) and 0 <= g < self.N:
                cap *= 4
                continue
            check(rc)
            return cols[:n.value], vals[:n.value]

    def to_csr(self):
        """Materialise (small problems only; used by tests)."""
        rp = np.zeros(self.N + 1, dtype=np.int64)
        cols, vals = [], []
        for g in range(self.N):
            c, v = self.row(g)
            cols.append(c)
            vals.append(v)
            rp[g + 1] = rp[g] + len(c)
        return rp, np.concatenate(cols).astype(IDX), np.concatenate(vals)

    def permute(self, part, P):
        """restricted_schwarz.cpp:105-152; returns (problem, perm, first_row)."""
        part = np.ascontiguousarray(part, dtype=np.uint32)
        perm = np.zeros(self.N, dtype=np.int64)
        fr = np.zeros(P + 1, dtype=np.int64)
        h = C.c_void_p()
        check(lib.schwz_problem_permute(self.h, P, ptr(part), ptr(perm), ptr(fr), C.byref(h)))
        return Problem(h), perm, fr

    def partition_graph(self, P):
        part = np.zeros(self.N, dtype=np.uint32)
        check(lib.schwz_partition_graph(self.h, P, ptr(part)))
        return part

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_problem_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def rhs_random(global_ids):
    """Initialize::generate_rhs (initialization.cpp:88-96) by global row id."""
    ids = np.ascontiguousarray(global_ids, dtype=np.int64)
    out = np.zeros(max(len(ids), 1), dtype=np.float64)
    check(lib.schwz_rhs_random(len(ids), ptr(ids), ptr(out)))
    return out[:len(ids)]


def partition_regular(N, P):
    fr = np.zeros(P + 1, dtype=np.int64)
    check(lib.schwz_partition_regular(N, P, ptr(fr)))
    return fr


def partition_regular2d(n1d, P):
    part = np.zeros(n1d * n1d, dtype=np.uint32)
    check(lib.schwz_partition_regular2d(n1d, P, ptr(part)))
    return part


class Subdomain:
    """One subdomain: host index sets + (after to_device) the HBM-resident
    iteration state.  Mirrors what SolverRAS::setup_local_matrices /
    setup_comm_buffers build (restricted_schwarz.cpp:56-604)."""

    batch_k = 0  # columns of the block state (batch_begin); 0: none

    def __init__(self, problem, P, me, overlap, first_row):
        self.problem = problem
        self.P, self.me, self.overlap = P, me, overlap
        self.first_row = np.ascontiguousarray(first_row, dtype=np.int64)
        h = C.c_void_p()
        check(lib.schwz_subdomain_setup(problem.h, P, me, overlap, ptr(self.first_row),
                                        C.byref(h)))
        self.h = h
        self.on_device = False
        self._sizes()

    def _sizes(self):
        s = np.zeros(10, dtype=np.int64)
        check(lib.schwz_subdomain_sizes(self.h, ptr(s)))
        (self.local_size, self.local_size_x, self.overlap_size, self.halo_size, self.nnz_local,
         self.nnz_interface, self.num_neighbors_in, self.num_neighbors_out, self.num_recv,
         self.num_send) = [int(v) for v in s]

    @property
    def local_to_global(self):
        out = np.zeros(self.local_size_x + self.halo_size, dtype=np.int64)
        check(lib.schwz_subdomain_local_to_global(self.h, ptr(out)))
        return out

    def local_matrix(self):
        rp = np.zeros(self.local_size_x + 1, dtype=IDX)
        col = np.zeros(max(self.nnz_local, 1), dtype=IDX)
        val = np.zeros(max(self.nnz_local, 1), dtype=np.float64)
        check(lib.schwz_subdomain_local_matrix(self.h, ptr(rp), ptr(col), ptr(val)))
        return rp, col[:self.nnz_local], val[:self.nnz_local]

    def interface_matrix(self):
        rp = np.zeros(self.local_size_x + 1, dtype=IDX)
        col = np.zeros(max(self.nnz_interface, 1), dtype=np.int64)
        val = np.zeros(max(self.nnz_interface, 1), dtype=np.float64)
        check(lib.schwz_subdomain_interface_matrix(self.h, ptr(rp), ptr(col), ptr(val)))
        return rp, col[:self.nnz_interface], val[:self.nnz_interface]

    def _list(self, fn, k):
        rank = C.c_int(0)
        cnt = C.c_int64(0)
        check(fn(self.h, k, C.byref(rank), C.byref(cnt), None))
        ids = np.zeros(max(cnt.value, 1), dtype=np.int64)
        check(fn(self.h, k, None, None, ptr(ids)))
        return rank.value, ids[:cnt.value]

    def get_lists(self):
        return [self._list(lib.schwz_subdomain_get_list, k) for k in range(self.num_neighbors_in)]

    def put_lists(self):
        return [self._list(lib.schwz_subdomain_put_list, k) for k in range(self.num_neighbors_out)]

    def add_put_list(self, p, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        check(lib.schwz_subdomain_add_put_list(self.h, p, len(ids), ptr(ids)))
        self._sizes()

    def send_offsets(self):
        out = []
        for k in range(self.num_neighbors_out + 1):
            o = C.c_int64(0)
            check(lib.schwz_subdomain_send_offset(self.h, k, C.byref(o)))
            out.append(o.value)
        return out

    def recv_offsets(self):
        out = []
        for k in range(self.num_neighbors_in + 1):
            o = C.c_int64(0)
            check(lib.schwz_subdomain_recv_offset(self.h, k, C.byref(o)))
            out.append(o.value)
        return out

    def local_rhs(self, rhs_fn):
        """[rhs[interior]; rhs[overlap_row]] (initialization.cpp:349-355);
        rhs_fn maps an array of global ids to values."""
        return np.ascontiguousarray(rhs_fn(self.local_to_global[:self.local_size_x]),
                                    dtype=np.float64)

    # ---- device -------------------------------------------------------------

    def to_device(self, local_rhs, local_solver=capi.SOLVER_ITERATIVE,
                  precond=capi.PRECOND_NONE, local_tol=1e-12, local_max_iters=-1,
                  natural_factor_ordering=False, spmv_variant=0, precond_block_size=1,
                  non_symmetric=False, restart_iter=1, par_ilu_sweeps=0, trisolve_sweeps=0):
        local_rhs = np.ascontiguousarray(local_rhs, dtype=np.float64)
        assert len(local_rhs) == self.local_size_x
        opt = capi.SolverOptions(local_solver, precond, local_tol, local_max_iters,
                                 int(natural_factor_ordering), spmv_variant, int(precond_block_size),
                                 int(bool(non_symmetric)), int(restart_iter), int(par_ilu_sweeps),
                                 int(trisolve_sweeps))
        check(lib.schwz_subdomain_to_device(self.h, ptr(local_rhs), C.byref(opt)))
        self.on_device = True

    def pack(self, d_send, stream=0):
        check(lib.schwz_ras_pack(self.h, ptr(d_send), _stream_arg(stream)))

    def unpack(self, d_recv, stream=0):
        check(lib.schwz_ras_unpack(self.h, ptr(d_recv), _stream_arg(stream)))

    def pack_f32(self, d_send, stream=0):
        check(lib.schwz_ras_pack_f32(self.h, ptr(d_send), _stream_arg(stream)))

    def unpack_f32(self, d_recv, stream=0):
        check(lib.schwz_ras_unpack_f32(self.h, ptr(d_recv), _stream_arg(stream)))

    def early_pack_ok(self):
        """Whether the local solver records the event pack_early waits for (CG with put lists)."""
        return bool(lib.schwz_ras_early_pack_ok(self.h))

    def pack_early(self, d_send, single=False, stream=0):
        """The pack of the NEXT exchange beside the tail of the running solve (schwz_ras_pack_early):
        `stream` waits until the rows of the put lists are final, then gathers them from the solve's result."""
        check(lib.schwz_ras_pack_early(self.h, ptr(d_send), int(bool(single)), _stream_arg(stream)))

    def pack_neighbor(self, k, dst, single=False, stream=0):
        """Out-neighbour k's halo values to the device address `dst` (its receive window)."""
        check(lib.schwz_ras_pack_neighbor(self.h, int(k), ptr(dst), int(bool(single)), _stream_arg(stream)))

    def unpack_neighbor(self, k, src, single=False, stream=0):
        """In-neighbour k's halo values from the device address `src` (its send window)."""
        check(lib.schwz_ras_unpack_neighbor(self.h, int(k), ptr(src), int(bool(single)), _stream_arg(stream)))

    def update_boundary(self, stream=0):
        check(lib.schwz_ras_update_boundary(self.h, _stream_arg(stream)))

    def local_residual(self, stream=0):
        out = C.c_double(0.0)
        check(lib.schwz_ras_local_residual(self.h, C.byref(out), _stream_arg(stream)))
        return out.value

    def local_residual_launch(self, stream=0):
        check(lib.schwz_ras_local_residual_launch(self.h, _stream_arg(stream)))

    def check_and_solve_launch(self, stream=0):
        check(lib.schwz_ras_check_and_solve_launch(self.h, _stream_arg(stream)))

    def norm_sq_to_device(self, d_ptr, stream=0):
        """Square of the last check residual norm to the device double at `d_ptr`, on `stream`, as soon as that
        scalar is final (the solve enqueued behind the check is not waited for)."""
        check(lib.schwz_ras_norm_sq_to_device(self.h, C.c_void_p(int(d_ptr)), _stream_arg(stream)))

    def local_residual_wait(self):
        out = C.c_double(0.0)
        check(lib.schwz_ras_local_residual_wait(self.h, C.byref(out)))
        return out.value

    def last_inner_stats(self):
        """(inner iterations, final residual norm) of the last local solve -- settings.enable_logging
        (solve.cpp:751-771); synchronises the device."""
        it, rn = C.c_int(0), C.c_double(0.0)
        check(lib.schwz_ras_last_inner_stats(self.h, C.byref(it), C.byref(rn)))
        return it.value, rn.value

    def set_local_max_iters(self, max_iters):
        """Inner iteration cap of later local solves (two-stage criterion, solve.cpp:723-742)."""
        check(lib.schwz_ras_set_local_max_iters(self.h, int(max_iters)))

    def set_local_precision(self, precision):
        """Precision of the iterative local solve from the next one on (schwz_ras_set_local_precision):
        capi.PRECISION_F64, or capi.PRECISION_F32 for the fp32 CG on the fp64 start residual."""
        check(lib.schwz_ras_set_local_precision(self.h, int(precision)))

    def local_precision(self):
        return int(lib.schwz_ras_local_precision(self.h))

    def set_nonsym_solver(self, which):
        """Krylov method of the iterative local solve of a non-symmetric matrix from the next solve on
        (schwz_ras_set_nonsym_solver): capi.NONSYM_GMRES (what to_device creates) or capi.NONSYM_BICGSTAB."""
        check(lib.schwz_ras_set_nonsym_solver(self.h, int(which)))

    def nonsym_solver(self):
        return int(lib.schwz_ras_nonsym_solver(self.h))

    def set_gmres_basis(self, which):
        """The type the local GMRES of a non-symmetric matrix stores its Krylov basis in
        (schwz_ras_set_gmres_basis): capi.GMRES_BASIS_F64 (what to_device creates) or capi.GMRES_BASIS_F32."""
        check(lib.schwz_ras_set_gmres_basis(self.h, int(which)))

    def gmres_basis(self):
        return int(lib.schwz_ras_gmres_basis(self.h))

    def set_sym_solver(self, which):
        """Method of the iterative local solve of a symmetric matrix from the next solve on
        (schwz_ras_set_sym_solver): capi.SYM_CG (what to_device creates) or capi.SYM_CHEBYSHEV."""
        check(lib.schwz_ras_set_sym_solver(self.h, int(which)))

    def sym_solver(self):
        return int(lib.schwz_ras_sym_solver(self.h))

    def cheb_bounds(self):
        """(lmin, lmax) of the subdomain's Chebyshev solver (after set_sym_solver(SYM_CHEBYSHEV))."""
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        check(lib.schwz_ras_cheb_bounds(self.h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def set_cheb_bounds(self, lmin, lmax):
        check(lib.schwz_ras_set_cheb_bounds(self.h, float(lmin), float(lmax)))

    def local_solve(self, stream=0, want_iters=False):
        it = C.c_int(0)
        check(lib.schwz_ras_local_solve(self.h, C.byref(it) if want_iters else None,
                                        _stream_arg(stream)))
        return it.value

    def restrict(self, stream=0):
        check(lib.schwz_ras_restrict(self.h, _stream_arg(stream)))

    def cg_flavour(self):
        """How the last local CG solve iterated (schwz_ras_cg_flavour: bits 0-1 launches per iteration,
        4 deferred x update, 8 / 16 z-sweep walk of the update / fused direction launch, 32 of the start)."""
        return int(lib.schwz_ras_cg_flavour(self.h))

    def y_form(self):
        """Where y lives (schwz_ras_y_form): 0 a buffer of its own, 1 the x~ buffer, 2 the other x~ buffer."""
        return int(lib.schwz_ras_y_form(self.h))

    def vector(self, which):
        p = C.c_void_p()
        n = C.c_int64(0)
        check(lib.schwz_ras_vector(self.h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def get_interior(self, stream=0):
        out = np.zeros(max(self.local_size, 1), dtype=np.float64)
        check(lib.schwz_ras_get_interior(self.h, ptr(out), _stream_arg(stream)))
        return out[:self.local_size]

    def true_residual_sq(self, stream=0):
        out = C.c_double(0.0)
        check(lib.schwz_ras_true_residual_sq(self.h, C.byref(out), _stream_arg(stream)))
        return out.value

    def apply_interior(self, d_out, stream=0):
        """(A x~) on the local_size interior rows to the device address d_out (x~ exchanged beforehand); the matrix
        pass of true_residual_sq with the vector kept (schwz_ras_apply_interior)."""
        check(lib.schwz_ras_apply_interior(self.h, ptr(d_out), _stream_arg(stream)))

    def algorithmic_bytes(self, which=0):
        return int(lib.schwz_ras_algorithmic_bytes(self.h, which))

    # ---- aggregation coarse correction (schwz_ras_coarse_*) ----------------------

    def coarse_set_aggregates(self, slot_agg, first_agg, m, nc):
        """Plans and uploads this subdomain's part of the coarse correction: `slot_agg` holds the global aggregate
        id of every x~ slot (local_size_x + halo), the subdomain owns the ids [first_agg, first_agg + m)."""
        slot_agg = np.ascontiguousarray(slot_agg, dtype=np.int32)
        assert len(slot_agg) == self.local_size_x + self.halo_size
        check(lib.schwz_ras_coarse_set_aggregates(self.h, ptr(slot_agg), int(first_agg), int(m), int(nc)))
        self._coarse_shape = (int(m), int(nc))

    def coarse_rows(self):
        """The subdomain's m rows of A0 = Z^T A Z as an (m, nc) array."""
        m, nc = self._coarse_shape
        out = np.zeros(max(m * nc, 1), dtype=np.float64)
        check(lib.schwz_ras_coarse_rows(self.h, ptr(out)))
        return out[:m * nc].reshape(m, nc)

    def coarse_residual(self, coarse, stream=0):
        check(lib.schwz_ras_coarse_residual(self.h, coarse.h, _stream_arg(stream)))

    def coarse_apply(self, coarse, stream=0):
        check(lib.schwz_ras_coarse_apply(self.h, coarse.h, _stream_arg(stream)))

    def aggregate_sums(self, coarse, d_vec, stream=0):
        """s[first_agg + a] = sum of d_vec over the rows of the subdomain's aggregate a, into s of `coarse`; d_vec: the
        integer address of at least local_size doubles in HBM, in local order (schwz_ras_aggregate_sums)."""
        check(lib.schwz_ras_aggregate_sums(self.h, coarse.h if coarse is not None else None, ptr(d_vec),
                                           _stream_arg(stream)))

    # ---- a new right-hand side on a set-up subdomain (schwz_ras_rhs_*, schwz_ras_restart) ----

    def rhs_set(self, rhs, stream=0):
        """The local right-hand side (vector id 3) from `rhs`: a host array of local_size_x values in local order,
        or the integer address of as many doubles in HBM."""
        if isinstance(rhs, np.ndarray):
            rhs = np.ascontiguousarray(rhs, dtype=np.float64)
            assert len(rhs) == self.local_size_x
            check(lib.schwz_ras_rhs_set(self.h, ptr(rhs), 0, _stream_arg(stream)))
        else:
            check(lib.schwz_ras_rhs_set(self.h, ptr(rhs), 1, _stream_arg(stream)))

    def rhs_index(self, index=None):
        """The map of rhs_gather: the global position of every local row's right-hand side (None: the subdomain's own
        local-to-global list).  Checked on the host here, uploaded by the first gather."""
        if index is not None:
            index = np.ascontiguousarray(index, dtype=np.int64)
            assert len(index) == self.local_size_x
        check(lib.schwz_ras_rhs_index(self.h, ptr(index)))

    def rhs_gather(self, d_global, n_global, stream=0):
        """The local right-hand side gathered from a global vector of n_global doubles in HBM."""
        check(lib.schwz_ras_rhs_gather(self.h, ptr(d_global), int(n_global), _stream_arg(stream)))

    def rhs_aggregate(self, stream=0):
        """beta of the coarse part recomputed from the local right-hand side (nothing without aggregates)."""
        check(lib.schwz_ras_rhs_aggregate(self.h, _stream_arg(stream)))

    def rhs_norm_sq(self, stream=0):
        """Sum of the squares of the right-hand side over the interior rows (waits for the stream)."""
        out = C.c_double(0.0)
        check(lib.schwz_ras_rhs_norm_sq(self.h, C.byref(out), _stream_arg(stream)))
        return out.value

    def rhs_norm_sq_local(self, stream=0):
        """The same over all local_size_x rows: the square of the check residual of a zero x~."""
        out = C.c_double(0.0)
        check(lib.schwz_ras_rhs_norm_sq_local(self.h, C.byref(out), _stream_arg(stream)))
        return out.value

    def restart(self, keep_x=False, stream=0):
        """The iteration state back to "just uploaded" (keep_x: every vector keeps its values); the solver objects
        forget their last solve either way (schwz_ras_restart)."""
        check(lib.schwz_ras_restart(self.h, int(bool(keep_x)), _stream_arg(stream)))

    # ---- the steps of a RAS iteration on block vectors (schwz_ras_batch_*): k columns, element (i, j) at i * k + j ----

    def batch_begin(self, k):
        """The block state of k = 2, 4 or 8 columns: vectors and a block CG of its own, beside the single-vector state."""
        check(lib.schwz_ras_batch_begin(self.h, int(k)))
        self.batch_k = int(k)

    def batch_end(self):
        check(lib.schwz_ras_batch_end(self.h))
        self.batch_k = 0

    def batch_rhs_set(self, rhs, stream=0):
        """rhs: host array of shape (local_size_x, k), local order; x~ and y go back to zero, b~ = b."""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        assert rhs.shape == (self.local_size_x, self.batch_k)
        check(lib.schwz_ras_batch_rhs_set(self.h, ptr(rhs), _stream_arg(stream)))

    def batch_pack(self, d_send, stream=0):
        check(lib.schwz_ras_batch_pack(self.h, ptr(d_send), _stream_arg(stream)))

    def batch_unpack(self, d_recv, stream=0):
        check(lib.schwz_ras_batch_unpack(self.h, ptr(d_recv), _stream_arg(stream)))

    def batch_update_boundary(self, stream=0):
        check(lib.schwz_ras_batch_update_boundary(self.h, _stream_arg(stream)))

    def batch_local_residual(self, stream=0):
        """Per column ||b~_j - A x~_j||_2 (waits for the stream)."""
        out = (C.c_double * self.batch_k)()
        check(lib.schwz_ras_batch_local_residual(self.h, out, _stream_arg(stream)))
        return list(out)

    def batch_local_solve(self, frozen=0, stream=0, want_iters=False):
        it = (C.c_int * self.batch_k)()
        check(lib.schwz_ras_batch_local_solve(self.h, int(frozen), it if want_iters else None, _stream_arg(stream)))
        return list(it)

    def batch_restrict(self, frozen=0, stream=0):
        check(lib.schwz_ras_batch_restrict(self.h, int(frozen), _stream_arg(stream)))

    def batch_vector(self, which):
        """(device pointer, length) of the block x~ (0), b~ (1), y (2) or b (3)."""
        p = C.c_void_p()
        n = C.c_int64(0)
        check(lib.schwz_ras_batch_vector(self.h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def batch_get_interior(self, stream=0):
        out = np.zeros((max(self.local_size, 1), self.batch_k), dtype=np.float64)
        check(lib.schwz_ras_batch_get_interior(self.h, ptr(out), _stream_arg(stream)))
        return out[:self.local_size]

    def batch_true_residual_sq(self, stream=0):
        out = (C.c_double * self.batch_k)()
        check(lib.schwz_ras_batch_true_residual_sq(self.h, out, _stream_arg(stream)))
        return list(out)

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_subdomain_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def dense_inverse(a):
    """Inverse of a dense square matrix on the host (schwz_dense_inverse: LU with partial pivoting); a singular
    matrix raises ERR_INVALID."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.ndim == 2 and a.shape[0] == a.shape[1]
    inv = np.zeros_like(a)
    check(lib.schwz_dense_inverse(a.shape[0], ptr(a), ptr(inv)))
    return inv


class Coarse:
    """The per-process part of the coarse correction on the device (schwz_coarse_create): the explicit inverse of
    A0, the coarse residual s and the correction c."""

    def __init__(self, inv):
        inv = np.ascontiguousarray(inv, dtype=np.float64)
        assert inv.ndim == 2 and inv.shape[0] == inv.shape[1]
        self.nc = int(inv.shape[0])
        h = C.c_void_p()
        check(lib.schwz_coarse_create(self.nc, ptr(inv), C.byref(h)))
        self.h = h

    def vector(self, which):
        """(device pointer, length) of s (which = 0) or c (1)."""
        p, n = C.c_void_p(), C.c_int32(0)
        check(lib.schwz_coarse_vector(self.h, int(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    def solve(self, stream=0):
        check(lib.schwz_coarse_solve(self.h, _stream_arg(stream)))

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_coarse_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Outer:
    """The device half of the outer FGMRES (schwz_outer_create): the basis V (restart + 1 columns), the preconditioned
    directions Z (restart columns), w and a copy of b, each over the n interior rows of the process's subdomains in
    subdomain order, and the vector passes of one outer iteration."""

    V, Z, W, B = 0, 1, 2, 3

    def __init__(self, n, restart, basis=None):
        """basis: None (schwz_outer_create), "double" or "single" (schwz_outer_create_basis: V in fp32)."""
        self.n, self.restart, self.basis = int(n), int(restart), basis or "double"
        h = C.c_void_p()
        if basis is not None and basis not in capi.OUTER_BASIS:
            raise capi.SchwzError(capi.ERR_INVALID, "Outer: basis must be 'double' or 'single', not %r" % (basis,))
        if basis is None:
            check(lib.schwz_outer_create(self.n, self.restart, C.byref(h)))
        else:
            check(lib.schwz_outer_create_basis(self.n, self.restart, capi.OUTER_BASIS[basis], C.byref(h)))
        self.h = h

    def basis_read(self, j, first, count, d_dst, stream=0):
        """d_dst[0:count] (fp64, any 8-byte alignment) = rows first .. first + count of V_j, widened exactly."""
        check(lib.schwz_outer_basis_read(self.h, int(j), int(first), int(count), ptr(d_dst), _stream_arg(stream)))

    def basis_write(self, j, first, count, d_src, stream=0):
        """Rows first .. first + count of V_j = d_src[0:count], rounded to nearest even on a single-basis object."""
        check(lib.schwz_outer_basis_write(self.h, int(j), int(first), int(count), ptr(d_src), _stream_arg(stream)))

    def residual(self, d_t, stream=0):
        """w = b - t for the n doubles at the device address d_t; returns w . w (waits for the stream)."""
        out = np.zeros(1)
        check(lib.schwz_outer_residual(self.h, ptr(d_t), ptr(out), _stream_arg(stream)))
        return float(out[0])

    def vector(self, which, j=0):
        """Device address of V_j (which = 0; ERR_INVALID on a single-basis object), Z_j (1), w (2) or the copy of b
        (3)."""
        p = C.c_void_p()
        check(lib.schwz_outer_vector(self.h, int(which), int(j), C.byref(p)))
        return p.value

    def start(self, inv_beta, stream=0):
        check(lib.schwz_outer_start(self.h, float(inv_beta), _stream_arg(stream)))

    def dots(self, j, stream=0):
        """[V_0 . w, ..., V_j . w, w . w] on the host (waits for the stream)."""
        out = np.zeros(j + 2)
        check(lib.schwz_outer_dots(self.h, int(j), ptr(out), _stream_arg(stream)))
        return out

    def project_dots(self, j, h, stream=0):
        """w -= sum_i h[i] V_i over i <= j; returns the dots of the new w like dots()."""
        h = np.ascontiguousarray(h, dtype=np.float64)
        assert len(h) >= j + 1
        out = np.zeros(j + 2)
        check(lib.schwz_outer_project_dots(self.h, int(j), ptr(h), ptr(out), _stream_arg(stream)))
        return out

    def normalize(self, j, inv_norm, stream=0):
        check(lib.schwz_outer_normalize(self.h, int(j), float(inv_norm), _stream_arg(stream)))

    def combine(self, y, d_x, stream=0):
        """x += sum_i y[i] Z_i at the device address d_x (n doubles)."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        check(lib.schwz_outer_combine(self.h, len(y), ptr(y), ptr(d_x), _stream_arg(stream)))

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.schwz_outer_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def outer_copy(n, d_src, d_dst, stream=0):
    """d_dst[0:n] = d_src[0:n] on the device, any 8-byte alignment (schwz_outer_copy)."""
    check(lib.schwz_outer_copy(int(n), ptr(d_src), ptr(d_dst), _stream_arg(stream)))


def lu(rp, col, val, natural=False):
    """Host sparse LU with threshold partial pivoting standing in for UMFPACK (solve.cpp:144-173):
    A(row_perm, col_perm) = L U, no row scaling."""
    rp = np.ascontiguousarray(rp, dtype=IDX)
    col = np.ascontiguousarray(col, dtype=IDX)
    val = np.ascontiguousarray(val, dtype=np.float64)
    n = len(rp) - 1
    out = [C.c_void_p() for _ in range(8)]
    check(lib.schwz_lu(n, ptr(rp), ptr(col), ptr(val), int(natural), *[C.byref(o) for o in out]))

    def take(p, cnt, ctype, dtype):
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(max(cnt, 1),))[:cnt].copy()
        return a.astype(dtype, copy=False)

    l_rp = take(out[0], n + 1, C.c_int32, IDX)
    u_rp = take(out[3], n + 1, C.c_int32, IDX)
    lnz, unz = (int(l_rp[-1]), int(u_rp[-1])) if n else (0, 0)
    res = dict(l_rp=l_rp, l_col=take(out[1], lnz, C.c_int32, IDX),
               l_val=take(out[2], lnz, C.c_double, np.float64), u_rp=u_rp,
               u_col=take(out[4], unz, C.c_int32, IDX),
               u_val=take(out[5], unz, C.c_double, np.float64),
               row_perm=take(out[6], n, C.c_int32, IDX),
               col_perm=take(out[7], n, C.c_int32, IDX))
    for o in out:
        lib.schwz_free(o)
    return res
