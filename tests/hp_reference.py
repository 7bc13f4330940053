"""Extended-precision references for the GPU tests, in plain numpy.

Everything here is written from the textbook statement of the operation (CSR row sums, forward / backward
substitution, right-preconditioned MGS-GMRES with Givens rotations, preconditioned CG, truncated Neumann series,
synchronous ParILU sweeps) and runs in `np.longdouble`, which has a 64-bit mantissa on x86 (eps = 1.08e-19): 11 bits
more than the float64 the kernels compute in, so a kernel's summation-order error of a few hundred ulp is
visible against it.  Where `np.longdouble` is no wider than float64 the functions call `pytest.skip`
instead of quietly comparing float64 with float64.

Most routines take a `dtype` argument so that the same text also runs in float64: the distance between the
two runs is what float64 rounding alone does to the result, and the GMRES tests size their tolerance from it.

Layout of triangular factors (the library's, `schwz.ilu0` / `schwz.Trs`): CSR, L holds its diagonal LAST in
each row, U holds it FIRST.
"""
import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53   # unit roundoff of float64


def require_extended_precision():
    """The one skip of the modules that import this file: no extended precision on this platform."""
    if np.finfo(LD).eps >= 2.0 ** -53:
        import pytest
        pytest.skip("np.longdouble is no wider than float64 on this platform")


def _guard(dtype):
    if np.dtype(dtype) == np.dtype(LD):
        require_extended_precision()


# ---- CSR row sums -------------------------------------------------------------------------------------

def _row_passes(rp):
    """For k = 0, 1, ...: the rows that own a k-th entry (row lengths sorted once)."""
    rp = np.asarray(rp, dtype=np.int64)
    ln = np.diff(rp)
    order = np.argsort(-ln, kind="stable")
    sorted_len = ln[order]
    k = 0
    while True:
        cnt = int(np.searchsorted(-sorted_len, -k, side="left"))   # rows with length > k
        if cnt == 0:
            return
        rows = order[:cnt]
        yield rows, rp[rows] + k
        k += 1


def spmv(rp, col, val, x, dtype=LD):
    """y = A x, every row summed entry by entry in CSR order, in `dtype`."""
    _guard(dtype)
    col = np.asarray(col, dtype=np.int64)
    val = np.asarray(val, dtype=dtype)
    x = np.asarray(x, dtype=dtype)
    y = np.zeros(len(rp) - 1, dtype=dtype)
    for rows, at in _row_passes(rp):
        y[rows] += val[at] * x[col[at]]
    return y


# ---- triangular factors -------------------------------------------------------------------------------

class Tri:
    """One triangular factor prepared for substitution: rows grouped into dependency levels, so that a solve
    is one vectorised pass per level (rows of a level are independent) with every row summed in CSR order
    (a level of one row: numpy's dot over the row)."""

    def __init__(self, rp, col, val, lower):
        self.rp = np.asarray(rp, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)
        self.val64 = np.asarray(val, dtype=np.float64)
        self.lower = bool(lower)
        self.n = n = len(self.rp) - 1
        rp_, col_ = self.rp, self.col
        dpos = rp_[1:] - 1 if lower else rp_[:-1].copy()
        assert n == 0 or np.array_equal(col_[dpos], np.arange(n)), "diagonal must be last in L, first in U"
        self.dpos = dpos
        self.s0 = rp_[:-1] if lower else rp_[:-1] + 1     # strict part of each row
        self.s1 = rp_[1:] - 1 if lower else rp_[1:]
        self.longest = int(np.diff(rp_).max()) if n else 0
        # levels: a python loop, once per factor
        level = [0] * n
        cl, s0l, s1l = col_.tolist(), self.s0.tolist(), self.s1.tolist()
        for i in (range(n) if lower else range(n - 1, -1, -1)):
            m = -1
            for j in range(s0l[i], s1l[i]):
                lv = level[cl[j]]
                if lv > m:
                    m = lv
            level[i] = m + 1
        level = np.asarray(level, dtype=np.int64)
        self.nlevels = int(level.max()) + 1 if n else 0
        order = np.argsort(level, kind="stable")
        bounds = np.searchsorted(level[order], np.arange(self.nlevels + 1))
        self.plan = []
        for lv in range(self.nlevels):
            rows = order[bounds[lv]:bounds[lv + 1]]
            if len(rows) == 1:   # a chain link or a long banded row: one dot product over the row's slice
                r = int(rows[0])
                self.plan.append((r, slice(int(self.s0[r]), int(self.s1[r]))))
                continue
            ln = self.s1[rows] - self.s0[rows]
            byl = np.argsort(-ln, kind="stable")
            rows, ln = rows[byl], ln[byl]
            passes = []
            for k in range(int(ln[0]) if len(ln) else 0):
                cnt = int(np.searchsorted(-ln, -k, side="left"))
                passes.append((cnt, self.s0[rows[:cnt]] + k))
            self.plan.append((rows, passes))

    def solve(self, b, dtype=LD, comparison=False):
        """T x = b by substitution in `dtype`.  comparison: with M(T) (|t_ii| on the diagonal, -|t_ij| off it)
        in place of T."""
        _guard(dtype)
        val = np.asarray(self.val64, dtype=dtype)
        if comparison:
            val = -np.abs(val)
            val[self.dpos] = -val[self.dpos]
        x = np.zeros(self.n, dtype=dtype)
        b = np.asarray(b, dtype=dtype)
        diag = val[self.dpos]
        xcol = self.col
        for rows, passes in self.plan:
            if isinstance(passes, slice):
                x[rows] = (b[rows] - np.dot(val[passes], x[xcol[passes]])) / diag[rows]
                continue
            s = b[rows].copy()
            for cnt, at in passes:
                s[:cnt] -= val[at] * x[self.col[at]]
            x[rows] = s / diag[rows]
        return x

    def abs_times(self, x, dtype=LD):
        """|T| |x| in `dtype`."""
        return spmv(self.rp, self.col, np.abs(np.asarray(self.val64, dtype=dtype)), np.abs(np.asarray(x, dtype=dtype)),
                    dtype)


def lower_solve(rp, col, val, b, dtype=LD):
    return Tri(rp, col, val, True).solve(b, dtype)


def upper_solve(rp, col, val, b, dtype=LD):
    return Tri(rp, col, val, False).solve(b, dtype)


def factors(f):
    """(Tri L, Tri U) from a dict with l_rp, l_col, l_val, u_rp, u_col, u_val (what schwz.ilu0 returns)."""
    return Tri(f["l_rp"], f["l_col"], f["l_val"], True), Tri(f["u_rp"], f["u_col"], f["u_val"], False)


def trs_apply(L, U, perm_in, perm_out, b, dtype=LD, parts=False):
    """w = b[perm_in]; L w1 = w; U w0 = w1; y[perm_out] = w0 (None: identity), what trs_create documents."""
    b = np.asarray(b, dtype=dtype)
    w = b if perm_in is None else b[np.asarray(perm_in, dtype=np.int64)]
    w1 = L.solve(w, dtype)
    w0 = U.solve(w1, dtype)
    if perm_out is None:
        y = w0
    else:
        y = np.zeros_like(w0)
        y[np.asarray(perm_out, dtype=np.int64)] = w0
    return (y, w1, w0) if parts else y


def trs_error_bound(L, U, x_L, x_U):
    """Componentwise forward-error bound of the two substitutions carried out in float64, rows summed in ANY
    order (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 8.5: the computed solution
    solves (T + dT) x = b with |dT| <= gamma_k |T|; with |T^-1| <= M(T)^-1 for the comparison matrix M(T)):

        e_L = k u M(L)^-1 |L| |x_L|,      e_U = M(U)^-1 (k u |U| |x_U| + e_L),

    k = longest row + 1, u = 2^-53.  Returned in the order of x_U (before the output permutation)."""
    k = max(L.longest, U.longest) + 1
    ku = LD(k) * LD(U64)
    e_L = L.solve(ku * L.abs_times(x_L), LD, comparison=True)
    return U.solve(ku * U.abs_times(x_U) + e_L, LD, comparison=True)


# ---- Jacobi-sweep triangular solves (trs_jacobi_kernel) ---------------------------------------------------

def _jacobi_factor(T, b, sweeps, dtype, e_b=None):
    """x_0 = D^-1 b, x_{m+1} = D^-1 (b - T_s x_m), `sweeps` times.  With e_b (a bound on the error already in
    b) also returns the running componentwise bound of a float64 evaluation: every pass adds (k + 2) u times
    the magnitudes that enter the row (k products and subtractions, the reciprocal diagonal, the final
    product) and propagates the previous pass's error through |D^-1| |T_s|."""
    val = np.asarray(T.val64, dtype=dtype)
    dinv = 1 / val[T.dpos]
    strict = val.copy()
    strict[T.dpos] = 0
    b = np.asarray(b, dtype=dtype)
    x = dinv * b
    if e_b is None:
        for _ in range(sweeps):
            x = dinv * (b - spmv(T.rp, T.col, strict, x, dtype))
        return x
    ku = LD(T.longest + 2) * LD(U64)
    adinv, astrict = np.abs(dinv), np.abs(strict)
    e = adinv * e_b + 2 * LD(U64) * np.abs(x)
    for _ in range(sweeps):
        mag = np.abs(b) + spmv(T.rp, T.col, astrict, np.abs(x), dtype)
        e = adinv * (e_b + spmv(T.rp, T.col, astrict, e, dtype) + ku * mag)
        x = dinv * (b - spmv(T.rp, T.col, strict, x, dtype))
    return x, e


def jacobi_sweep_solve(L, U, b, sweeps, dtype=LD, bound=False):
    """y = U^-1 L^-1 b with each factor applied by the truncated Neumann series of trs_jacobi_kernel.
    bound: also the derived componentwise error bound of a float64 evaluation (see _jacobi_factor)."""
    _guard(dtype)
    if not bound:
        return _jacobi_factor(U, _jacobi_factor(L, b, sweeps, dtype), sweeps, dtype)
    zero = np.zeros(L.n, dtype=dtype)
    r, e_r = _jacobi_factor(L, b, sweeps, dtype, zero)
    return _jacobi_factor(U, r, sweeps, dtype, e_r)


# ---- preconditioner applications --------------------------------------------------------------------------

def precond_none(dtype=LD):
    return lambda v: np.array(v, dtype=dtype)


def precond_jacobi(rp, col, val, dtype=LD):
    rp = np.asarray(rp, dtype=np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    on = np.asarray(col) == rows
    d = np.zeros(len(rp) - 1, dtype=dtype)
    d[rows[on]] = np.asarray(val, dtype=dtype)[on]
    return lambda v: np.asarray(v, dtype=dtype) / d


def precond_block_jacobi(rp, col, val, block_ptr, dtype=LD):
    """Dense inverses of the diagonal blocks block_ptr[k]:block_ptr[k+1], formed in longdouble by Gauss-Jordan
    elimination with partial pivoting (numpy.linalg has no longdouble; all blocks of one size are eliminated
    together), applied in `dtype`."""
    _guard(LD)
    rp = np.asarray(rp, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(rp) - 1
    block_ptr = np.asarray(block_ptr, dtype=np.int64)
    sizes = np.diff(block_ptr)
    rows = np.repeat(np.arange(n), np.diff(rp))
    blk = np.searchsorted(block_ptr, rows, side="right") - 1
    inside = (col >= block_ptr[blk]) & (col < block_ptr[blk + 1])
    groups = []
    for s in np.unique(sizes):
        ks = np.nonzero(sizes == s)[0]
        slot = np.full(len(sizes), -1, dtype=np.int64)
        slot[ks] = np.arange(len(ks))
        e = np.nonzero(inside & (slot[blk] >= 0))[0]
        exact64 = np.asarray(val).dtype == np.float64
        dense = np.zeros((len(ks), s, s), dtype=np.float64 if exact64 else LD)
        dense[slot[blk[e]], rows[e] - block_ptr[blk[e]], col[e] - block_ptr[blk[e]]] = np.asarray(val)[e]
        idx = block_ptr[ks][:, None] + np.arange(s)[None, :]
        if exact64:   # equal blocks (a stencil matrix has a handful) are eliminated once: the same operations per block
            seen, back = {}, np.empty(len(ks), dtype=np.int64)
            for k, blk_k in enumerate(dense):
                back[k] = seen.setdefault(blk_k.tobytes(), len(seen))
            first = np.full(len(seen), -1, dtype=np.int64)
            first[back[::-1]] = np.arange(len(ks))[::-1]
            inv = _dense_inverse(dense[first].astype(LD)).reshape(-1, s, s)[back]
        else:
            inv = _dense_inverse(dense).reshape(-1, s, s)
        groups.append((idx, inv.astype(dtype)))

    def apply(v):
        v = np.asarray(v, dtype=dtype)
        out = np.empty(n, dtype=dtype)
        for idx, inv in groups:
            out[idx] = np.einsum("kij,kj->ki", inv, v[idx])
        return out
    return apply


def _dense_inverse(a):
    """Inverses of a stack of square matrices (K, s, s), or of one (s, s), in longdouble."""
    single = a.ndim == 2
    w = np.asarray(a, dtype=LD).reshape((-1,) + a.shape[-2:])
    K, s = w.shape[0], w.shape[1]
    w = np.concatenate([w, np.broadcast_to(np.eye(s, dtype=LD), (K, s, s))], axis=2)
    ar = np.arange(K)
    for c in range(s):
        p = c + np.argmax(np.abs(w[:, c:, c]), axis=1)
        rc, rp_ = w[ar, c].copy(), w[ar, p].copy()
        w[ar, p], w[ar, c] = rc, rp_
        w[:, c] /= w[:, c, c][:, None]
        f = w[:, :, c].copy()
        f[:, c] = 0
        w -= f[:, :, None] * w[:, c][:, None, :]
    inv = w[:, :, s:]
    return inv[0] if single else inv


def precond_ilu(f, dtype=LD):
    """z = U^-1 L^-1 v by substitution on given factors (schwz.ilu0's)."""
    L, U = factors(f)
    return lambda v: U.solve(L.solve(v, dtype), dtype)


def precond_isai(schwz, f, dtype=LD):
    """z = W_U (W_L v): the incomplete sparse approximate inverses of given factors on the factors' own patterns,
    two CSR products."""
    wl = schwz.isai(f["l_rp"], f["l_col"], f["l_val"], True)
    wu = schwz.isai(f["u_rp"], f["u_col"], f["u_val"], False)
    return lambda v: spmv(f["u_rp"], f["u_col"], wu, spmv(f["l_rp"], f["l_col"], wl, v, dtype), dtype)


def make_precond(schwz, oracle, rp, col, val, precond, bs, dtype):
    """The preconditioner codes of the library (0 none, 1 Jacobi, 2 block-Jacobi, 3 ILU, 4 ISAI) as hp_reference
    applications; the block partition is the oracle's (structure only), the ILU(0) factors and the ISAI values on
    their patterns the library's (host code: schwz.ilu0, schwz.isai)."""
    if precond == 0:
        return precond_none(dtype)
    if precond == 1 or (precond == 2 and bs == 1):
        return precond_jacobi(rp, col, val, dtype)
    if precond == 2:
        return precond_block_jacobi(rp, col, val, oracle.jacobi_blocks(rp, col, bs), dtype)
    if precond == 4:
        return precond_isai(schwz, schwz.ilu0(rp, col, val), dtype)
    assert precond == 3
    return precond_ilu(schwz.ilu0(rp, col, val), dtype)


# ---- the Dirichlet Laplacian by array slicing, dot products, preconditioned CG ---------------------------------

def stencil_apply(x, shape, dtype=LD):
    """y = A x for the 5- / 7-point Laplacian with Dirichlet boundaries on a grid of shape (nx, ny[, nz]) in natural
    order, x fastest (diagonal 2 * dim, off-diagonals -1), by array slicing.  The terms of a row are added in
    ascending column order, as spmv adds them from a CSR with sorted columns: in float64 the two agree bit for
    bit.  A tenth of the time of the row passes of spmv, which is what makes references at 2^24 rows affordable."""
    _guard(dtype)
    dims = tuple(int(s) for s in shape)[::-1]          # slowest axis first
    v = np.asarray(x, dtype=dtype).reshape(dims)
    nd = len(dims)
    y = np.zeros(dims, dtype=dtype)

    def cut(ax, a, b):
        return tuple(slice(a, b) if k == ax else slice(None) for k in range(nd))
    for ax in range(nd):                                # columns below the diagonal: the farthest first
        y[cut(ax, 1, None)] -= v[cut(ax, None, -1)]
    y += np.dtype(dtype).type(2 * nd) * v
    for ax in range(nd - 1, -1, -1):                    # columns above it: the nearest first
        y[cut(ax, None, -1)] -= v[cut(ax, 1, None)]
    return y.reshape(-1)


def slab_operator(local_to_global, nx, ny, dtype=LD):
    """v -> A_loc v for the local matrix of a z-slab subdomain of the 7-point Laplacian on an nx x ny x nz grid: the
    rows of the subdomain (interior and overlap, local_to_global[:local_size_x]) fill a box of whole x-y planes,
    A_loc is the Dirichlet Laplacian of that box in the subdomain's numbering.  The vector is put into natural
    order, the slicing stencil applied, the result brought back."""
    g = np.asarray(local_to_global, dtype=np.int64)
    plane = int(nx) * int(ny)
    lo = int(g.min())
    nz, rem = divmod(int(g.max()) + 1 - lo, plane)
    assert lo % plane == 0 and rem == 0 and len(g) == nz * plane and len(np.unique(g)) == len(g), "not a box of planes"
    pos = g - lo

    def apply(v):
        w = np.empty(len(pos), dtype=dtype)
        w[pos] = v
        return stencil_apply(w, (nx, ny, nz), dtype)[pos]
    return apply


def dot(x, y):
    """sum_i x_i y_i by numpy's pairwise summation (np.sum), in the type of the operands.  Not `@` / np.dot: for
    longdouble those accumulate in sequence, and at 2^24 terms lose the digits the CG tests are about."""
    return np.sum(x * y)


def pcg(rp, col, val, b, x0, precond_apply, iters, rtol=0.0, dtype=LD, keep=None):
    """Preconditioned conjugate gradients (Hestenes & Stiefel 1952; Saad, Iterative Methods, Alg. 9.1) with the
    stopping rule schwz_pcg_solve documents: before every update the recurred residual norm is tested against
    rtol times the start residual norm, at most `iters` updates; rtol <= 0 runs exactly `iters` updates (a residual
    of exactly zero ends the solve all the same: there is no direction left).

    `rp` is a CSR row pointer (with col, val) or a callable v -> A v in `dtype` (col and val are then ignored).
    Returns (x, hist): hist[k] = ||r_k||_2 from the recurrence r_{k+1} = r_k - alpha_k A p_k, len(hist) - 1 the
    number of updates.  keep: a dict whose keys are update counts; x after that many updates is stored in it."""
    _guard(dtype)
    A = rp if callable(rp) else (lambda v: spmv(rp, col, val, v, dtype))
    b = np.asarray(b, dtype=dtype)
    x = np.array(x0, dtype=dtype) if x0 is not None else np.zeros(len(b), dtype=dtype)
    r = b - A(x)
    rr = dot(r, r)
    r0 = np.sqrt(rr)
    hist = [r0]
    z = precond_apply(r)
    p = np.array(z, dtype=dtype)
    rho = dot(r, z)
    if keep is not None and 0 in keep:
        keep[0] = x.copy()
    for k in range(iters):
        if np.sqrt(rr) <= np.dtype(dtype).type(rtol) * r0:
            break
        q = A(p)
        alpha = rho / dot(p, q)
        x += alpha * p
        r -= alpha * q
        z = precond_apply(r)
        rho_new = dot(r, z)
        rr = dot(r, r)
        p *= rho_new / rho
        p += z
        rho = rho_new
        hist.append(np.sqrt(rr))
        if keep is not None and k + 1 in keep:
            keep[k + 1] = x.copy()
    return x, hist


# ---- GMRES ----------------------------------------------------------------------------------------------------

def gmres(rp, col, val, b, x0, precond_apply, iters, restart, rtol=0.0, dtype=LD):
    """Restarted GMRES(restart), right preconditioned, modified Gram-Schmidt, Givens rotations (Saad &
    Schultz 1986), at most `iters` Krylov vectors, with the structure of schwz_gmres_solve: the stop tests at
    the top of a cycle use the true residual, inside a cycle the rotated right-hand side.

    Returns (x, hist): hist[0] is the initial residual norm, hist[k] the residual norm reported after k
    Krylov vectors (if a cycle top stops the solve, its true residual norm replaces the last entry).
    len(hist) - 1 is the iteration count."""
    _guard(dtype)
    m = max(int(restart), 1)
    n = len(rp) - 1
    b = np.asarray(b, dtype=dtype)
    x = np.array(x0, dtype=dtype) if x0 is not None else np.zeros(n, dtype=dtype)
    V = np.zeros((m + 1, n), dtype=dtype)
    H = np.zeros((m + 1, m), dtype=dtype)
    cs, sn = np.zeros(m, dtype=dtype), np.zeros(m, dtype=dtype)
    hist = []
    it, r0 = 0, None
    while True:
        r = b - spmv(rp, col, val, x, dtype)
        beta = np.sqrt(np.dot(r, r))
        if r0 is None:
            r0 = beta
            hist.append(beta)
        else:
            hist[-1] = beta
        if it >= iters or beta <= rtol * r0 or beta == 0:
            break
        V[0] = r / beta
        g = np.zeros(m + 1, dtype=dtype)
        g[0] = beta
        k = 0
        resn = beta
        for j in range(m):
            if it >= iters:
                break
            w = spmv(rp, col, val, precond_apply(V[j]), dtype)
            for i in range(j + 1):
                H[i, j] = np.dot(w, V[i])
                w = w - H[i, j] * V[i]
            hn = np.sqrt(np.dot(w, w))
            H[j + 1, j] = hn
            V[j + 1] = w / hn if hn != 0 else 0
            for i in range(j):
                t = cs[i] * H[i, j] + sn[i] * H[i + 1, j]
                H[i + 1, j] = -sn[i] * H[i, j] + cs[i] * H[i + 1, j]
                H[i, j] = t
            if H[j + 1, j] == 0:
                cs[j], sn[j] = 1, 0
            else:
                rr = np.hypot(H[j, j], H[j + 1, j])
                cs[j], sn[j] = H[j, j] / rr, H[j + 1, j] / rr
            H[j, j] = cs[j] * H[j, j] + sn[j] * H[j + 1, j]
            H[j + 1, j] = 0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            it += 1
            k = j + 1
            resn = abs(g[j + 1])
            hist.append(resn)
            if resn <= rtol * r0:
                break
        y = np.zeros(k, dtype=dtype)
        for i in range(k - 1, -1, -1):
            y[i] = (g[i] - np.dot(H[i, i + 1:k], y[i + 1:k])) / H[i, i]
        t = np.zeros(n, dtype=dtype)
        for i in range(k):
            t = t + y[i] * V[i]
        x = x + precond_apply(t)
        if resn <= rtol * r0 or it >= iters:
            break
    return x, hist


# ---- synchronous ParILU sweeps (schwz.parilu) ---------------------------------------------------------------

class Pattern:
    """The ILU(0) pattern of A in the library's layout (L: strict lower + unit diagonal LAST, U: upper with
    its diagonal FIRST) and, for every entry of A, the (L index, U index) pairs of its ParILU sum."""

    def __init__(self, rp, col):
        n = len(rp) - 1
        self.n = n
        rows = [dict((int(col[j]), j) for j in range(rp[i], rp[i + 1])) for i in range(n)]
        l_rp, u_rp, l_col, u_col = [0], [0], [], []
        self.where = np.zeros(rp[-1], dtype=np.int64)   # target index in L (>= 0 below the diagonal) or U
        self.is_l = np.zeros(rp[-1], dtype=bool)
        for i in range(n):
            for j in range(rp[i], rp[i + 1]):
                c = int(col[j])
                if c < i:
                    self.where[j], self.is_l[j] = len(l_col), True
                    l_col.append(c)
                else:
                    self.where[j] = len(u_col)
                    u_col.append(c)
            l_col.append(i)
            l_rp.append(len(l_col))
            u_rp.append(len(u_col))
        self.l_rp, self.l_col = np.array(l_rp), np.array(l_col)
        self.u_rp, self.u_col = np.array(u_rp), np.array(u_col)
        self.pairs = []
        self.pivot = np.zeros(rp[-1], dtype=np.int64)
        for i in range(n):
            for j in range(rp[i], rp[i + 1]):
                c = int(col[j])
                ps = []
                for k in sorted(rows[i]):
                    if k >= min(i, c):
                        break
                    q = rows[k].get(c)
                    if q is not None:
                        ps.append((self.where[rows[i][k]], self.where[q]))
                self.pairs.append(ps)
                if c < i:
                    self.pivot[j] = self.where[rows[c][c]]
        self.rp = np.asarray(rp)

    def depth(self):
        """Longest dependency chain among the entries (row-major order lists dependencies first)."""
        d = np.zeros(len(self.pairs), dtype=np.int64)
        l_of = {}
        u_of = {}
        for e in range(len(self.pairs)):
            (l_of if self.is_l[e] else u_of)[self.where[e]] = e
        for e, ps in enumerate(self.pairs):
            m = 0
            for li, ui in ps:
                m = max(m, d[l_of[li]], d[u_of[ui]])
            if self.is_l[e]:
                m = max(m, d[u_of[self.pivot[e]]])
            d[e] = m + 1
        return int(d.max())


def parilu_numpy(pat, val, sweeps):
    """Synchronous ParILU sweeps from L0 = strict lower part of A + unit diagonal, U0 = upper part."""
    lv = np.ones(len(pat.l_col))
    uv = np.zeros(len(pat.u_col))
    lv[pat.where[pat.is_l]] = val[pat.is_l]
    uv[pat.where[~pat.is_l]] = val[~pat.is_l]
    for _ in range(sweeps):
        ln, un = lv.copy(), uv.copy()
        for e, ps in enumerate(pat.pairs):
            s = val[e]
            for li, ui in ps:
                s -= lv[li] * uv[ui]
            if pat.is_l[e]:
                ln[pat.where[e]] = s / uv[pat.pivot[e]]
            else:
                un[pat.where[e]] = s
        lv, uv = ln, un
    return lv, uv


# ---- triangular factors built in numpy (inputs of the triangular-solve tests) -----------------------------------

def _values(n, rp, col, lower, rng, rho):
    """Values for a triangular pattern (diagonal last in a lower, first in an upper row): off-diagonal entries
    random with sum_j |t_ij| = rho |t_ii| (row diagonally dominant: M(T) is well conditioned), diagonals in
    +-[1, 2]."""
    ln = np.diff(rp)
    val = rng.uniform(0.25, 1.0, rp[-1]) * rng.choice([-1.0, 1.0], rp[-1])
    dpos = rp[1:] - 1 if lower else rp[:-1]
    strict = np.ones(rp[-1], dtype=bool)
    strict[dpos] = False
    d = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    rowid = np.repeat(np.arange(n), ln)
    tot = np.bincount(rowid[strict], weights=np.abs(val[strict]), minlength=n)
    val[strict] *= (rho * np.abs(d) / np.maximum(tot, 1e-300))[rowid[strict]]
    val[dpos] = d
    return val


def _assemble(n, rows_l, rows_u, rng, rho):
    """Factors in the library's layout from per-row strict column lists."""
    out = {}
    for name, rows, lower in (("l", rows_l, True), ("u", rows_u, False)):
        ln = np.array([len(r) for r in rows], dtype=np.int64) + 1
        rp = np.concatenate([[0], np.cumsum(ln)])
        col = np.empty(rp[-1], dtype=np.int64)
        dpos = rp[1:] - 1 if lower else rp[:-1]
        strict = np.ones(rp[-1], dtype=bool)
        strict[dpos] = False
        col[dpos] = np.arange(n)
        if strict.any():
            col[strict] = np.concatenate([np.sort(np.asarray(r, dtype=np.int64)) for r in rows])
        out[name + "_rp"], out[name + "_col"] = rp.astype(np.int32), col.astype(np.int32)
        out[name + "_val"] = _values(n, rp, col, lower, rng, rho)
    return out


def five_point_factors(n, nx, rng, rho=0.4):
    """The pattern of the ILU(0) of a five-point stencil on a grid nx wide (natural order, the last grid line
    may be incomplete): L holds south and west, U east and north."""
    i = np.arange(n, dtype=np.int64)
    south, west = i >= nx, (i % nx) > 0
    east, north = ((i % nx) < nx - 1) & (i + 1 < n), i + nx < n
    out = {}
    l_rp = np.concatenate([[0], np.cumsum(south.astype(np.int64) + west + 1)])
    l_col = np.empty(l_rp[-1], dtype=np.int64)
    l_col[l_rp[:-1][south]] = i[south] - nx
    l_col[(l_rp[:-1] + south)[west]] = i[west] - 1
    l_col[l_rp[1:] - 1] = i
    u_rp = np.concatenate([[0], np.cumsum(1 + east.astype(np.int64) + north)])
    u_col = np.empty(u_rp[-1], dtype=np.int64)
    u_col[u_rp[:-1]] = i
    u_col[(u_rp[:-1] + 1)[east]] = i[east] + 1
    u_col[(u_rp[:-1] + 1 + east)[north]] = i[north] + nx
    for name, rp, col, lower in (("l", l_rp, l_col, True), ("u", u_rp, u_col, False)):
        out[name + "_rp"], out[name + "_col"] = rp.astype(np.int32), col.astype(np.int32)
        out[name + "_val"] = _values(n, rp, col, lower, rng, rho)
    return out


def diagonal_factors(n, rng):
    return _assemble(n, [[]] * n, [[]] * n, rng, 0.0)


def bidiagonal_factors(n, rng, rho=0.4):
    """One dependency chain: row i of L needs row i - 1, row i of U row i + 1."""
    return _assemble(n, [[k - 1] if k else [] for k in range(n)], [[k + 1] if k + 1 < n else [] for k in range(n)],
                     rng, rho)


def layered_rows(widths, rng, deps=2, long_row=None):
    """Strict lower rows whose dependency levels have exactly the given widths: a row of layer q > 0 takes one
    column in layer q - 1 and up to deps - 1 more among all earlier rows.  long_row = (layer, count): the first
    row of that layer takes `count` distinct earlier columns instead."""
    start = np.concatenate([[0], np.cumsum(widths)])
    rows = []
    for q, w in enumerate(widths):
        for k in range(w):
            if q == 0:
                rows.append([])
                continue
            cols = {int(rng.integers(start[q - 1], start[q]))}
            want = deps
            if long_row is not None and long_row[0] == q and k == 0:
                want = long_row[1]
            while len(cols) < min(want, start[q]):
                cols.add(int(rng.integers(0, start[q])))
            rows.append(sorted(cols))
    return rows


def layered_factors(widths, rng, deps=2, long_row=None, rho=0.4):
    """L with the level widths given; U the same kind of structure mirrored (row i -> n - 1 - i), so that its
    levels, counted from the last row, have the same widths."""
    n = int(np.sum(widths))
    rows_l = layered_rows(widths, rng, deps, long_row)
    mirrored = layered_rows(widths, rng, deps, long_row)
    rows_u = [[n - 1 - c for c in mirrored[n - 1 - i]] for i in range(n)]
    return _assemble(n, rows_l, rows_u, rng, rho)


def banded_factors(n, lo, hi, rng, rho=0.4):
    """Dense-ish banded factors: row i of L takes column i - 1 and, in all, between lo and hi of the columns
    [i - hi - 40, i) (as many as exist near the corner), U is the mirror image: one row per level, rows far
    longer than a wave."""
    def rows():
        out = []
        for i in range(n):
            first = max(0, i - hi - 40)
            cnt = min(int(rng.integers(lo, hi + 1)), i - first)
            picks = first + rng.choice(i - 1 - first, size=cnt - 1, replace=False) if cnt > 1 else []
            out.append(np.append(picks, i - 1).astype(np.int64) if cnt else [])
        return out
    rows_l, m = rows(), rows()
    rows_u = [n - 1 - np.asarray(m[n - 1 - i], dtype=np.int64) for i in range(n)]
    return _assemble(n, rows_l, rows_u, rng, rho)


def rescale(f, rng, span=20):
    """Row and column scalings by signed powers of two, T -> D1 T D2 with |d| in [2^-span, 2^span] on the
    diagonal of the result: non-unit, negative, badly scaled pivots, while M(T) = |D1| M(T0) |D2| keeps the
    conditioning of the comparison matrix that the componentwise bound depends on.  Exact in float64."""
    n = len(f["l_rp"]) - 1
    out = dict(f)
    for name in ("l", "u"):
        rp, col = f[name + "_rp"].astype(np.int64), f[name + "_col"].astype(np.int64)
        e1, e2 = rng.integers(-span // 2, span // 2 + 1, n), rng.integers(-span // 2, span // 2 + 1, n)
        d1 = np.ldexp(rng.choice([-1.0, 1.0], n), e1)
        d2 = np.ldexp(1.0, e2)
        rowid = np.repeat(np.arange(n), np.diff(rp))
        out[name + "_val"] = f[name + "_val"] * d1[rowid] * d2[col]
    return out


# ---- row-wise bounds of CSR row sums evaluated in float64 ------------------------------------------------------------
# Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: a sum of k products evaluated in
# floating point with unit roundoff u, in ANY order of the additions, with or without FMA, is
#     s^ = sum_j a_j x_j (1 + theta_j),   |theta_j| <= gamma(k) = k u / (1 - k u)
# (every product is rounded at most once and then takes part in at most k - 1 rounded additions; an FMA rounds once
# where a product and an addition round twice).  Each further rounded operation on the result raises the index of
# gamma by one (Lemma 3.3).  Nothing below is measured on a kernel.  The bounds assume that no product underflows.
#
# The references are longdouble evaluations of the same sums, themselves rounded: by the same argument with
# u_ld = 2^-64 their error is at most (k + 2) u_ld times the same magnitudes (to first order, which at 2^-64 leaves
# a factor 1 + 1e-15 that the "+ 2" absorbs for every k used here).  Every bound below carries that term.

U_LD = 2.0 ** -64   # unit roundoff of the x87 extended format


def gamma(k, u=U64):
    """gamma(k) = k u / (1 - k u), in longdouble; k a number or an array."""
    ku = np.asarray(k, dtype=LD) * LD(u)
    return ku / (1 - ku)


def abs_row_sums(rp, col, val, x):
    """m_i = sum_j |a_ij| |x_j| in longdouble."""
    return spmv(rp, col, np.abs(np.asarray(val, dtype=LD)), np.abs(np.asarray(x, dtype=LD)), LD)


def axpby(rp, col, val, x, alpha, beta, y0, dtype=LD):
    """y = alpha A x + beta y0, rows summed in CSR order, in `dtype`.  beta == 0: y0 is not looked at (it may hold
    NaN), which is what BLAS and schwz_csr_spmv document."""
    t = np.dtype(dtype).type
    y = t(alpha) * spmv(rp, col, val, x, dtype)
    if beta != 0:
        y = y + t(beta) * np.asarray(y0, dtype=dtype)
    return y


def axpby_bound(rp, col, val, x, alpha, beta, y0):
    """Row-wise bound of a float64 evaluation of y = alpha A x + beta y0 against axpby(...) in longdouble:

        |y^_i - y_i| <= gamma(k_i + 2) (|alpha| m_i + |beta| |y0_i|)  +  (k_i + 2) 2^-64 (the same magnitudes),

    k_i the stored entries of row i.  Derivation: s^_i carries gamma(k_i) (above); alpha s^_i, beta y0_i and their
    sum are three more rounded operations, of which a term passes through two: gamma(k_i + 2) on the first term,
    gamma(2) <= gamma(k_i + 2) on the second.  Valid for any order of the k_i additions, with or without FMA."""
    k = np.diff(np.asarray(rp, dtype=np.int64))
    mag = abs(LD(alpha)) * abs_row_sums(rp, col, val, x)
    if beta != 0:
        mag = mag + abs(LD(beta)) * np.abs(np.asarray(y0, dtype=LD))
    return (gamma(k + 2) + (k + 2) * LD(U_LD)) * mag


def residual(rp, col, val, x, b, dtype=LD):
    """r = b - A x, rows summed in CSR order, in `dtype`."""
    return np.asarray(b, dtype=dtype) - spmv(rp, col, val, x, dtype)


def residual_bound(rp, col, val, x, b):
    """e_i with |r^_i - r_i| <= e_i for a float64 evaluation of r_i = b_i - (A x)_i against residual(...) in
    longdouble:  e_i = gamma(k_i + 1) (|b_i| + m_i) + (k_i + 2) 2^-64 (|b_i| + m_i): the k_i roundings of the row sum
    and the subtraction.  The interface update b~_i = b_i - (A_Gamma x~)_i is the same expression."""
    k = np.diff(np.asarray(rp, dtype=np.int64))
    mag = np.abs(np.asarray(b, dtype=LD)) + abs_row_sums(rp, col, val, x)
    return (gamma(k + 1) + (k + 2) * LD(U_LD)) * mag


def norm_sq_bound(r, e, L, root=False):
    """B with |S^ - rho^2| <= B, where rho^2 = sum_{i<L} r_i^2 in longdouble (np.sum) and S^ is that sum formed in
    float64 from computed residuals r^_i with |r^_i - r_i| <= e_i, in ANY order -- per-workgroup partial sums folded
    by another kernel included:

        B = sum_{i<L} (2 |r_i| e_i + e_i^2)  +  (gamma(L + 1) + (L + 1) 2^-64) sum_{i<L} (|r_i| + e_i)^2.

    First term: |r^_i^2 - r_i^2| = |r^_i - r_i| |r^_i + r_i| <= e_i (2 |r_i| + e_i).  Second: each square is rounded
    once and passes through at most L - 1 rounded additions (a sum with an exact zero, the rows past L, rounds
    nothing), so S^ = sum r^_i^2 (1 + theta_i) with |theta_i| <= gamma(L) <= gamma(L + 1), and r^_i^2 <=
    (|r_i| + e_i)^2; the reference's own sum adds (L + 1) 2^-64 of the same.  (e from residual_bound already holds
    the rounding of the reference residuals.)

    root: the API returned v = fl(sqrt(S^)) and the test compares v^2 (squared in longdouble) with rho^2: v^2 =
    S^ (1 + d)^2, |d| <= u, so 4 u rho^2 is added (it covers (2 u + u^2) (rho^2 + B) as long as B < rho^2 / 2,
    which the callers assert)."""
    r = np.abs(np.asarray(r, dtype=LD)[:L])
    e = np.asarray(e, dtype=LD)[:L]
    B = np.sum(2 * r * e + e * e) + (gamma(L + 1) + (L + 1) * LD(U_LD)) * np.sum((r + e) ** 2)
    if root:
        rho2 = np.sum(r * r)
        assert B < rho2 / 2
        B = B + 4 * LD(U64) * rho2
    return B


# ---- the tile rule of schwz_csr_create, and which branch of spmv_tiled2_kernel a tile takes -----------------------------

TILE_ROWS, TILE_NNZ = 256, 2048   # kTileRows, kTileNnz


def tiles_of(rp):
    """Row boundaries of the tiles: consecutive rows, at most 256 of them, at most 2046 entries; a longer row forms a
    tile of its own (the loop of schwz_csr_create)."""
    rp = np.asarray(rp, dtype=np.int64)
    n = len(rp) - 1
    out, r = [0], 0
    while r < n:
        e = r
        while e < n and e - r < TILE_ROWS and rp[e + 1] - rp[r] <= TILE_NNZ - 2:
            e += 1
        e = max(e, r + 1)
        out.append(e)
        r = e
    return np.asarray(out, dtype=np.int64)


def tile_branches(rp):
    """Per tile "a" (16-byte aligned window), "b" (fits the tile but not the aligned window: unaligned staging) or
    "c" (one long row reduced by the workgroup), by the conditions of spmv_tiled2_kernel."""
    rp = np.asarray(rp, dtype=np.int64)
    t = tiles_of(rp)
    out = []
    for r0, r1 in zip(t[:-1], t[1:]):
        s, cnt = rp[r0], rp[r1] - rp[r0]
        out.append("a" if (s & 3) + cnt <= TILE_NNZ else ("b" if r1 - r0 > 1 else "c"))
    return out


def stream_cap(rp):
    """The masked-add form of the straight-line kernel of spmv_stream.hip (8, 16 or 32 entries per row), 0 where it
    does not apply: a row of more than 32 entries or a tile outside the aligned window."""
    longest = int(np.diff(np.asarray(rp, dtype=np.int64)).max()) if len(rp) > 1 else 0
    if len(rp) < 2 or longest > 32 or any(b != "a" for b in tile_branches(rp)):
        return 0
    return 32 if longest > 16 else (16 if longest > 8 else 8)


# ---- seeded matrices of the row-sum tests --------------------------------------------------------------------------

def csr_from_lengths(lens, ncols, rng):
    """Random CSR with the given row lengths: distinct sorted columns, standard normal values."""
    lens = np.asarray(lens, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = np.empty(rp[-1], dtype=np.int32)
    for i, ln in enumerate(lens):
        if ln:
            col[rp[i]:rp[i + 1]] = np.sort(rng.choice(ncols, size=ln, replace=False))
    return rp.astype(np.int32), col, rng.standard_normal(rp[-1])


def short_lengths(n, max_len, rng):
    lens = rng.integers(0, max_len + 1, size=n)
    lens[rng.integers(0, n, size=max(n // 10, 1))] = 0
    return lens


def laplacian(shape):
    """The 5- / 7-point Dirichlet Laplacian of stencil_apply as CSR with sorted columns (natural order, x fastest)."""
    import scipy.sparse as sp
    a = None
    for k, m in enumerate(shape):
        t = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m), format="csr")
        term = t
        for q, mq in enumerate(shape):
            if q < k:
                term = sp.kron(term, sp.identity(mq, format="csr"), format="csr")
            elif q > k:
                term = sp.kron(sp.identity(mq, format="csr"), term, format="csr")
        a = term if a is None else a + term
    a = a.tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def window2049_lengths(rng, tail=300, tail_len=6):
    """Row 0 has 1027 entries and rows 1 and 2 have 1023 each: row 1 does not fit behind row 0 (2050 > 2046), so
    tile 1 starts at entry 1027 = 3 mod 4 and holds rows 1 and 2, 2046 entries: (s & 3) + cnt = 2049 > 2048, the
    unaligned staging branch with two rows.  (With 3 entries in row 0 the greedy rule would take row 1 into tile 0.)
    Then `tail` short rows, the first of them not empty (it ends tile 1), some of the others empty."""
    tail_lens = short_lengths(tail, tail_len, rng)
    tail_lens[0] = max(tail_lens[0], 1)
    return np.concatenate([[1027, 1023, 1023], tail_lens])


def scaled_matrix(n, max_len, rng, span=40, band=None):
    """Ragged rows of at most max_len entries (some empty), row i scaled by 2^s_i and column j by 2^t_j, s and t in
    [-span, span]: exact in float64.  Returns (rp, col, val, s, t).  band: columns within that distance of the row."""
    lens = short_lengths(n, max_len, rng)
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = np.empty(rp[-1], dtype=np.int32)
    for i, ln in enumerate(lens):
        if ln:
            if band is None:
                col[rp[i]:rp[i + 1]] = np.sort(rng.choice(n, size=ln, replace=False))
            else:
                lo, hi = max(0, i - band), min(n, i + band + 1)
                col[rp[i]:rp[i + 1]] = lo + np.sort(rng.choice(hi - lo, size=ln, replace=False))
    s, t = rng.integers(-span, span + 1, n), rng.integers(-span, span + 1, n)
    rowid = np.repeat(np.arange(n), lens)
    val = np.ldexp(rng.standard_normal(rp[-1]), s[rowid] + t[col])
    return rp.astype(np.int32), col, val, s, t


def rowsum_case(name):
    """The stand-alone SpMV cases: dict(rp, col, val, ncols, x, y0, branches), seeded by name.  `branches`: the
    branches of spmv_tiled2_kernel the matrix is built to reach (asserted by the tests through tile_branches)."""
    rng = np.random.default_rng(sum(name.encode()) + 1000)
    want, y_exp = set("a"), None
    if name == "window2049":
        ncols = 1100
        rp, col, val = csr_from_lengths(window2049_lengths(rng), ncols, rng)
        want = {"a", "b"}
    elif name == "longrows":
        # long rows between short ones; the pad row in front of each long row sets its start modulo 4 (2047 fits the
        # aligned window from 0 or 1, 2048 from 0 only; a second row of 2047 starts at 3 and takes branch c)
        ncols = 5200
        lens = []
        for ln, mod in ((5000, 0), (2046, None), (2047, 1), (2048, 0), (2049, 2), (2047, 3), (2500, None)):
            if lens:
                lens += list(rng.integers(1, 9, size=5))
                if mod is not None:
                    lens.append(1 + (mod - (sum(lens) + 1)) % 4)
            lens.append(ln)
        rp, col, val = csr_from_lengths(lens, ncols, rng)
        want = {"a", "c"}
    elif name in ("scaled8", "scaled16", "scaled32"):
        n = 1501
        rp, col, val, s, _ = scaled_matrix(n, int(name[6:]), rng)
        ncols, y_exp = n, s
    elif name == "rect_wide":
        ncols = 1900
        rp, col, val = csr_from_lengths(short_lengths(700, 24, rng), ncols, rng)
    elif name == "rect_tall":
        ncols = 700
        rp, col, val = csr_from_lengths(short_lengths(1900, 24, rng), ncols, rng)
    elif name == "lap3d":
        rp, col, val = laplacian((23, 17, 11))
        ncols = len(rp) - 1
    elif name == "lap2d":
        rp, col, val = laplacian((97, 97))
        ncols = len(rp) - 1
    elif name == "ani4_crop":
        import os
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ani4_crop.npz"))
        rp, col, val = g["rp"], g["col"], g["val"]
        ncols = len(rp) - 1
    elif name == "one":
        rp, col, val, ncols = np.array([0, 1], np.int32), np.array([0], np.int32), np.array([-1.75]), 1
    elif name == "three":
        rp, col, val, ncols = np.array([0, 2, 2, 3], np.int32), np.array([0, 2, 1], np.int32), rng.standard_normal(3), 3
    else:
        raise KeyError(name)
    n = len(rp) - 1
    x = rng.standard_normal(ncols)
    y0 = rng.standard_normal(n)
    if y_exp is not None:
        y0 = np.ldexp(y0, y_exp)      # of the size of its row: an order-1 y0 would hide a small row behind beta y0
    return dict(name=name, rp=rp, col=col, val=val, ncols=ncols, x=x, y0=y0, branches=want)


ROWSUM_CASES = ("window2049", "longrows", "scaled8", "scaled16", "scaled32", "rect_wide", "rect_tall", "lap3d",
                "lap2d", "ani4_crop", "one", "three")
ALPHA_BETA = ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0), (0.0, 1.0))


# ---- seeded matrices of the RAS step tests: structurally symmetric, nonzero diagonal ------------------------------------

def sym_band_matrix(n, picks, band, rng, spd=True):
    """Row i takes up to `picks` columns in (i, i + band], the transposed entries are added, and the diagonal: at
    most 2 * picks + 1 entries in a row... of which the lower ones depend on the rows above (callers that need a cap
    assert it).  spd: symmetric values in (-1, 1) with diag = 1 + sum |off-diagonal| (strictly dominant, positive:
    SPD); otherwise independent standard normal values, a diagonal of magnitude >= 1."""
    import scipy.sparse as sp
    rows, cols = [], []
    for i in range(n - 1):
        hi = min(n, i + band + 1)
        k = min(int(rng.integers(0, picks + 1)), hi - i - 1)
        if k:
            c = i + 1 + rng.choice(hi - i - 1, size=k, replace=False)
            rows += [i] * k
            cols += list(c)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if spd:
        v = rng.uniform(-1.0, 1.0, len(rows))
        a = sp.csr_matrix((v, (rows, cols)), shape=(n, n))
        a = a + a.T
        a = a + sp.diags(1.0 + np.asarray(abs(a).sum(axis=1)).ravel())
    else:
        a = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(n, n))
        a = a + sp.csr_matrix((rng.standard_normal(len(rows)), (cols, rows)), shape=(n, n))
        a = a + sp.diags(rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n))
    a = a.tocsr()
    a.sort_indices()
    assert a.nnz == 2 * len(rows) + n    # no entry cancelled: the structure is symmetric
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def rescale_rows_cols(rp, col, val, rng, span=40):
    """D1 A D2 with powers of two in [2^-span, 2^span]: exact.  Returns (val, s, t)."""
    n = len(rp) - 1
    s, t = rng.integers(-span, span + 1, n), rng.integers(-span, span + 1, n)
    rowid = np.repeat(np.arange(n), np.diff(rp))
    return np.ldexp(val, s[rowid] + t[col]), s, t


def arrow_matrix(n, rng):
    """Row 0 and column 0 dense, a tridiagonal rest, a dominant diagonal; symmetric."""
    import scipy.sparse as sp
    i = np.arange(1, n)
    v0 = rng.uniform(-1.0, 1.0, n - 1)
    v1 = rng.uniform(-1.0, 1.0, n - 2)
    a = sp.csr_matrix((np.concatenate([v0, v1]), (np.concatenate([np.zeros(n - 1, dtype=np.int64), i[:-1]]),
                                                   np.concatenate([i, i[1:]]))), shape=(n, n))
    a = a + a.T
    a = (a + sp.diags(1.0 + np.asarray(abs(a).sum(axis=1)).ravel())).tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def window2049_square(rng, n=1100):
    """window2049_lengths as a square, structurally symmetric matrix with a nonzero diagonal: rows 0, 1, 2 hold each
    other, themselves and 1024 / 1020 / 1020 of the columns from 3 on; row j >= 3 holds its diagonal, j - 1 and j + 1
    (from 3 on) and whichever of 0, 1, 2 hold it: at most 6 entries."""
    import scipy.sparse as sp
    rows, cols = [], []
    for r, cnt in ((0, 1024), (1, 1020), (2, 1020)):
        c = 3 + np.sort(rng.choice(n - 3, size=cnt, replace=False))
        rows += [r] * cnt + list(c)
        cols += list(c) + [r] * cnt
    for r in range(3):
        for c in range(3):
            rows.append(r), cols.append(c)
    j = np.arange(3, n)
    rows += list(j) + list(j[:-1]) + list(j[1:])
    cols += list(j) + list(j[1:]) + list(j[:-1])
    pat = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    pat.sum_duplicates()
    pat.sort_indices()
    val = rng.standard_normal(pat.nnz)
    rowid = np.repeat(np.arange(n), np.diff(pat.indptr))
    on = pat.indices == rowid
    val[on] = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n)
    return pat.indptr.astype(np.int32), pat.indices.astype(np.int32), val


# ---- the coarse correction (csrc/coarse.hip): residual of the aggregates, dense GEMV, apply --------------------------------

COARSE_PIECE_CAP = 2048   # kCoarsePieceCap: W entries one workgroup reduces


def pow2_operands(rng, n, lo=0, hi=0, exps=None):
    """+-u 2^e with u uniform in [0.5, 2) and e drawn from [lo, hi] (or given): no operand is small against its
    neighbours of the same exponent, which standard normal operands cannot promise over millions of products."""
    e = rng.integers(lo, hi + 1, n) if exps is None else np.asarray(exps)
    return np.ldexp(rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n), e)


def coarse_residual(rp, col, val, x, b, agg, m, dtype=LD):
    """s_a = sum_{i in a} (b_i - sum_j A_ij x~_j), a = agg[i] in [0, m), over the rows of (rp, col, val) -- the
    interior rows of a subdomain, columns index x~ -- from the definition: every row's residual in CSR order, the
    rows of an aggregate added in ascending order, in `dtype`.  No W is formed."""
    r = residual(rp, col, val, x, b, dtype)
    s = np.zeros(m, dtype=dtype)
    np.add.at(s, np.asarray(agg, dtype=np.int64), r)
    return s


def coarse_residual_bound(rp, col, val, x, b, agg, m):
    """e_a with |s^_a - s_a| <= e_a for a float64 evaluation of the coarse residual as beta_a - sum_j W_aj x~_j,
    W_aj = sum_{i in a} A_ij and beta_a = sum_{i in a} b_i formed first, against coarse_residual(...) in longdouble:

        e_a = (gamma(K_a + 1) + (K_a + 2) 2^-64) (sum_{i in a} |b_i| + sum_{i in a} sum_j |A_ij| |x~_j|),

    K_a = the rows of a plus their stored entries.  Derivation (Higham 3.1, as above): a value A_ij reaches s^_a
    through the additions inside W_aj (c_j - 1 of them, c_j the entries of a in column j), one product, the additions
    that join the n_W products of the aggregate into one number -- any tree over n_W leaves has n_W - 1 of them; an
    addition to an exact zero (a lane without an entry, the fold's start) rounds nothing -- and the subtraction from
    beta_a: c_j + n_W <= entries + 1 <= K_a rounded operations, since the n_W slots are distinct and slot j holds
    c_j - 1 entries more than one.  A b_i passes rows - 1 additions and the subtraction: rows <= K_a.  So every term
    carries at most gamma(K_a), and gamma(K_a + 1) bounds any order of these sums: the host plan's, the strided lanes
    and the tree of block_sum, the fold in table order.  A W_aj that sums to an exact zero and is dropped is the same
    statement with that sum.  The reference passes every term through at most k_i + 1 + rows <= K_a + 1 longdouble
    roundings: the second term.  Nothing is measured on a kernel."""
    rp = np.asarray(rp, dtype=np.int64)
    agg = np.asarray(agg, dtype=np.int64)
    K = np.zeros(m, dtype=np.int64)
    np.add.at(K, agg, 1 + np.diff(rp))
    mag = np.zeros(m, dtype=LD)
    np.add.at(mag, agg, np.abs(np.asarray(b, dtype=LD)) + abs_row_sums(rp, col, val, x))
    return (gamma(K + 1) + (K + 2) * LD(U_LD)) * mag


def coarse_w(rp, col, val, b, agg, m):
    """The host plan of the coarse residual restated (plan_coarse of coarse_plan.cpp) in float64: per aggregate the
    slots in ascending order with W_aj summed row after row, exact zeros dropped, and beta_a summed over the rows in
    ascending order.  Returns (w_ptr, w_slot, w_val, beta)."""
    rp = np.asarray(rp, dtype=np.int64)
    n = len(rp) - 1
    agg = np.asarray(agg, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)[:rp[n]]
    val = np.asarray(val, dtype=np.float64)[:rp[n]]
    a_of = np.repeat(agg, np.diff(rp))
    ncols = int(col.max()) + 1 if len(col) else 1
    key = a_of * ncols + col
    order = np.argsort(key, kind="stable")          # rows of a slot stay in ascending order
    key, v = key[order], val[order]
    start = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0] if len(key) else np.zeros(0, dtype=np.int64)
    gp = np.concatenate([start, [len(key)]]).astype(np.int64)
    w = spmv(gp, np.zeros(len(key), dtype=np.int64), v, np.ones(1), np.float64) if len(key) else np.zeros(0)
    keep = w != 0.0
    gkey = key[start][keep]
    w_val, w_slot, w_agg = w[keep], gkey % ncols, gkey // ncols
    w_ptr = np.zeros(m + 1, dtype=np.int64)
    np.add.at(w_ptr, w_agg + 1, 1)
    w_ptr = np.cumsum(w_ptr)
    row_order = np.argsort(agg, kind="stable")
    bp = np.zeros(m + 1, dtype=np.int64)
    np.add.at(bp, agg + 1, 1)
    beta = spmv(np.cumsum(bp), np.zeros(n, dtype=np.int64), np.asarray(b, dtype=np.float64)[row_order], np.ones(1),
                np.float64)
    return w_ptr, w_slot, w_val, beta


def coarse_pieces(w_ptr, cap=COARSE_PIECE_CAP):
    """[(aggregate, begin, end)] in table order and piece_ptr: an aggregate's W entries cut every `cap` entries."""
    pieces, piece_ptr = [], [0]
    for a in range(len(w_ptr) - 1):
        for b0 in range(int(w_ptr[a]), int(w_ptr[a + 1]), cap):
            pieces.append((a, b0, min(b0 + cap, int(w_ptr[a + 1]))))
        piece_ptr.append(len(pieces))
    return pieces, np.asarray(piece_ptr, dtype=np.int64)


def block_tree_sum64(t):
    """A workgroup's reduction of the float64 terms t restated: 256 lanes each add their share k, k + 256, ..., the
    64 lanes of a wave fold by halves (offsets 32 .. 1), the four waves as (w0 + w1) + (w2 + w3)."""
    lanes = np.zeros(256)
    t = np.asarray(t, dtype=np.float64)
    for k0 in range(0, len(t), 256):
        part = t[k0:k0 + 256]
        lanes[:len(part)] += part
    w = lanes.reshape(4, 64).copy()
    off = 32
    while off:
        w[:, :off] += w[:, off:2 * off]
        off >>= 1
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def coarse_residual64(w_ptr, w_slot, w_val, beta, x, pieces=None, piece_ptr=None, piece_sum=block_tree_sum64):
    """The device's evaluation restated in float64: one partial sum per piece (piece_sum), the pieces of an aggregate
    folded in table order, s_a = beta_a - t.  `pieces`, `piece_ptr`: another table (the seeded defects)."""
    if pieces is None:
        pieces, piece_ptr = coarse_pieces(w_ptr)
    t = np.asarray(w_val, dtype=np.float64) * np.asarray(x, dtype=np.float64)[w_slot]
    partial = np.array([piece_sum(t[b0:b1]) for _, b0, b1 in pieces] + [0.0])
    s = np.zeros(len(beta))
    for a in range(len(beta)):
        f = 0.0
        for p in range(int(piece_ptr[a]), int(piece_ptr[a + 1])):
            f += partial[p]
        s[a] = beta[a] - f
    return s


def aggregates_by_w_count(rp, col, targets):
    """One aggregate id per row: aggregate k < len(targets) is a contiguous row range whose rows hold exactly
    targets[k] distinct columns, the ranges in ascending row order; every other row belongs to the last aggregate,
    len(targets).  Found row by row: a range grows until it holds targets[k] columns; one more row adds about one
    column, but also none or two, and where the count steps over the target the range starts one row later (the row
    left out joins the last aggregate).  Asserts that every target is met exactly and that rows are left over."""
    rp = np.asarray(rp, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(rp) - 1

    def end_of(r0, t):
        seen, cnt = np.zeros(int(col.max()) + 1, dtype=bool), 0
        for r in range(r0, n):
            c = col[rp[r]:rp[r + 1]]
            cnt += int((~seen[c]).sum())
            seen[c] = True
            if cnt >= t:
                return r + 1 if cnt == t else None
        return None

    agg = np.full(n, len(targets), dtype=np.int64)
    r0 = 0
    for k, t in enumerate(targets):
        r1 = None
        while r1 is None:
            assert r0 < n, ("no contiguous row range with exactly %d columns" % t)
            r1 = end_of(r0, t)
            r0 += r1 is None
        agg[r0:r1] = k
        r0 = r1
    assert (agg == len(targets)).any()
    return agg


def coarse_gemv(M, s, dtype=LD, block=256):
    """(c, mag) with c = M s and mag_i = sum_j |M_ij| |s_j|, in `dtype`, in blocks of rows (nc = 4096 stays cheap)."""
    _guard(dtype)
    M = np.asarray(M)
    n = M.shape[0]
    sv = np.asarray(s, dtype=dtype)
    c, mag = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for i0 in range(0, n, block):
        p = M[i0:i0 + block].astype(dtype) * sv
        c[i0:i0 + block] = p.sum(axis=1)
        mag[i0:i0 + block] = np.abs(p).sum(axis=1)
    return c, mag


def coarse_gemv_bound(mag, nc):
    """Row bound of a float64 evaluation of c_i = sum_j M_ij s_j against coarse_gemv(...) in longdouble, mag_i =
    sum_j |M_ij| |s_j|:  (gamma(nc) + (nc + 2) 2^-64) mag_i -- nc products, each rounded once and passing at most
    nc - 1 rounded additions in ANY order (64 strided lanes folded by halves, 16-byte pairs, pairwise), with or
    without FMA; the reference's own sum adds the second term."""
    return (gamma(nc) + (nc + 2) * LD(U_LD)) * np.asarray(mag, dtype=LD)


def coarse_apply(x, y, c, slot_agg):
    """The apply is one rounded addition per entry, so its reference is exact: (x~ + c[agg], y + c[agg[:len(y)]]) in
    float64, to be compared bit for bit."""
    slot_agg = np.asarray(slot_agg, dtype=np.int64)
    c = np.asarray(c, dtype=np.float64)
    return np.asarray(x, dtype=np.float64) + c[slot_agg], np.asarray(y, dtype=np.float64) + c[slot_agg[:len(y)]]
