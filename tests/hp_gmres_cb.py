"""Extended-precision reference of the compressed-basis GMRES (csrc/gmres.hip, SCHWZ_GMRES_BASIS_F32), built on
hp_reference: the statement of the algorithm the solver documents, line for line, in `np.longdouble` or (the same
text) in float64.  fl32() is rounding to fp32 and widening back; it happens at exactly two points.

    nu = none
    cycle:
      r = b - A x ;  beta = ||r|| ;  nu = beta in the first cycle
      top:  stop if it == max_iters, or beta <= rtol nu, or beta == 0
      v_0 = fl32(r / beta) ;  g = beta e_1                                              (rounding point 1)
      for j = 0 .. m - 1, while it < max_iters
        w  = A M^-1 v_j                          (v_j is the ROUNDED vector)
        h  = V_j^T w                             pass A   (V_j = [v_0 .. v_j])
        w  = w - V_j h ;  h' = V_j^T w           pass B
        w  = w - V_j h' ;  eta = ||w||           pass C
        H(0..j, j) = h + h' ;  H(j+1, j) = eta
        v_{j+1} = fl32(w / eta), or 0 if eta == 0                                       (rounding point 2)
        the old Givens rotations on column j, the new one, g rotated ;  it += 1
        resn = |g_{j+1}| ;  leave the cycle AND the solve if resn <= rtol nu
      H y = g by back substitution ;  x += M^-1 (V y)
      stop if it == max_iters
"""
import numpy as np

import hp_reference as hp

LD = hp.LD


def fl32(v, dtype):
    return np.asarray(v, dtype=np.float32).astype(dtype)


def gmres_cb(rp, col, val, b, x0, precond_apply, iters, restart, rtol=0.0, dtype=LD, round_basis=True,
             add_second=True, rounded_to_spmv=True, cycle_starts=None):
    """Returns (x, hist) like hp_reference.gmres: hist[0] the start residual norm, hist[k] the residual norm the
    stop test saw after k Krylov vectors (a cycle top that stops the solve replaces the last entry by its true
    norm); len(hist) - 1 is the iteration count.  The three switches exist for the tests of this restatement
    only: the same text without the rounding, without h' in H, or with the unrounded vector in the product.
    `cycle_starts`: a list that receives (it, beta) of every cycle that ran.

    What the rounding costs inside one cycle: r = beta v_0 + e with |e| <= 2^-24 beta (every entry of r / beta moves
    by at most half an fp32 ulp), and e is outside what the cycle minimises, so at the end of a cycle
    |true residual| <= |recurred| + 2^-24 beta (1 + O(eps)) -- cycle_bound()."""
    hp._guard(dtype)
    m = max(int(restart), 1)
    n = len(rp) - 1
    b = np.asarray(b, dtype=dtype)
    x = np.array(x0, dtype=dtype) if x0 is not None else np.zeros(n, dtype=dtype)
    V = np.zeros((m + 1, n), dtype=dtype)
    H = np.zeros((m + 1, m), dtype=dtype)
    cs, sn = np.zeros(m, dtype=dtype), np.zeros(m, dtype=dtype)
    rnd = (lambda v: fl32(v, dtype)) if round_basis else (lambda v: v)
    hist = []
    it, r0 = 0, None
    while True:
        r = b - hp.spmv(rp, col, val, x, dtype)
        beta = np.sqrt(hp.dot(r, r))
        if r0 is None:
            r0 = beta
            hist.append(beta)
        else:
            hist[-1] = beta
        if it >= iters or beta <= rtol * r0 or beta == 0:
            break
        if cycle_starts is not None:
            cycle_starts.append((it, beta))
        vexact = r / beta
        V[0] = rnd(vexact)
        g = np.zeros(m + 1, dtype=dtype)
        g[0] = beta
        k = 0
        resn = beta
        for j in range(m):
            if it >= iters:
                break
            Vj = V[:j + 1]
            w = hp.spmv(rp, col, val, precond_apply(V[j] if rounded_to_spmv else vexact), dtype)
            h1 = np.sum(Vj * w, axis=1)
            w = w - np.sum(h1[:, None] * Vj, axis=0)
            h2 = np.sum(Vj * w, axis=1)
            w = w - np.sum(h2[:, None] * Vj, axis=0)
            hn = np.sqrt(hp.dot(w, w))
            H[:j + 1, j] = h1 + h2 if add_second else h1
            H[j + 1, j] = hn
            vexact = w / hn if hn != 0 else np.zeros(n, dtype=dtype)
            V[j + 1] = rnd(vexact)
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
        x = x + precond_apply(np.sum(y[:, None] * V[:k], axis=0))
        if resn <= rtol * r0 or it >= iters:
            break
    return x, hist


def cycle_bound(hist, cycle_starts):
    """Bound on the true relative residual of the returned x from the restatement's own figures: the recurred
    norm it stopped on plus 2^-24 of the last cycle's start residual, over the start residual of the solve."""
    if not cycle_starts:
        return float(hist[-1] / hist[0]) if hist[0] != 0 else 0.0
    return float((hist[-1] + 2.0 ** -24 * cycle_starts[-1][1]) / hist[0])


def true_relres(rp, col, val, x, b, x0=None):
    """||b - A x|| / ||b - A x0|| in np.longdouble (x0 = 0 when None)."""
    b = np.asarray(b, dtype=LD)
    r = b - hp.spmv(rp, col, val, np.asarray(x, dtype=LD), LD)
    r0 = b if x0 is None else b - hp.spmv(rp, col, val, np.asarray(x0, dtype=LD), LD)
    den = np.sqrt(hp.dot(r0, r0))
    num = np.sqrt(hp.dot(r, r))
    return float(num / den) if den != 0 else float(num)
