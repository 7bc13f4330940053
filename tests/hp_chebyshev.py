"""Extended-precision reference of the device-resident Chebyshev iteration (csrc/chebyshev.hip), built on
hp_reference: the statement of the algorithm the solver documents, line for line, in `np.longdouble` or (the same
text) in float64.

For SPD A, with M = I or M = diag(A), the spectrum of M^-1 A assumed in [lmin, lmax]:
    theta = (lmax + lmin) / 2 ;  delta = (lmax - lmin) / 2 ;  sigma = theta / delta

    r_0 = b - A x_0 ;  rho_0 = 1 / sigma ;  d_0 = (1 / theta) M^-1 r_0
    for k = 0 ... m-1:
        x_{k+1} = x_k + d_k
        r_{k+1} = r_k - A d_k
        rho_{k+1} = 1 / (2 sigma - rho_k)
        d_{k+1} = (rho_{k+1} rho_k) d_k + (2 rho_{k+1} / delta) M^-1 r_{k+1}

The scalars are computed in float64 in exactly this order whatever `dtype` is: they are the host's, passed to the
launches by value.  M^-1 r is dinv * r with dinv = 1 / diag rounded once, as the solver stores it.
With rtol > 0 the solve looks at ||r_k|| for k = 0 (mod CHECK_EVERY) and for k = m and returns x_k for the first such
k with ||r_k|| <= rtol ||r_0|| or ||r_k|| == 0; with rtol <= 0 it runs m corrections whatever the norms are.
"""
import numpy as np

import hp_reference as hp

LD = hp.LD
CHECK_EVERY = 8   # SCHWZ_CHEB_CHECK_EVERY


def diagonal(rp, col, val):
    """diag(A) in float64 (the last stored diagonal entry of a row, as the solver takes it)."""
    rp = np.asarray(rp, dtype=np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    on = np.asarray(col) == rows
    d = np.zeros(len(rp) - 1, dtype=np.float64)
    d[rows[on]] = np.asarray(val, dtype=np.float64)[on]
    return d


def gershgorin(rp, col, val, diag=None):
    """max_i |dinv_i| sum_j |a_ij| in float64, the row sums in CSR order (dinv = 1 without `diag`)."""
    rp = np.asarray(rp, dtype=np.int64)
    s = hp.spmv(rp, col, np.abs(np.asarray(val, dtype=np.float64)), np.ones(len(rp) - 1), np.float64)
    dinv = np.ones(len(rp) - 1) if diag is None else 1.0 / np.asarray(diag, dtype=np.float64)
    return float(np.max(np.abs(dinv) * s))


def scalars(lmin, lmax, m):
    """(1 / theta, [(a_k, c_k) for k = 1 ... m]) in float64: launch k computes d_k = a_k d_{k-1} + c_k M^-1 r_k."""
    lmin, lmax = np.float64(lmin), np.float64(lmax)
    theta = (lmax + lmin) / np.float64(2.0)
    delta = (lmax - lmin) / np.float64(2.0)
    sigma = theta / delta
    rho = np.float64(1.0) / sigma
    out = []
    for _ in range(m):
        rho_next = np.float64(1.0) / (np.float64(2.0) * sigma - rho)
        out.append((rho_next * rho, np.float64(2.0) * rho_next / delta))
        rho = rho_next
    return np.float64(1.0) / theta, out


def chebyshev(rp, col, val, b, x0, diag, lmin, lmax, iters, rtol=0.0, dtype=LD):
    """At most `iters` corrections.  diag: diag(A) for M = diag(A), None for M = I.
    Returns (x, hist): hist[k] = ||r_k|| from the recurrence (hist[0] the start residual norm), len(hist) - 1 the
    number of corrections applied."""
    hp._guard(dtype)
    t_ = np.dtype(dtype).type
    A = lambda w: hp.spmv(rp, col, val, w, dtype)   # noqa: E731
    b = np.asarray(b, dtype=dtype)
    x = np.array(x0, dtype=dtype) if x0 is not None else np.zeros(len(b), dtype=dtype)
    dinv = None if diag is None else (1.0 / np.asarray(diag, dtype=np.float64)).astype(dtype)
    Minv = (lambda v: v) if dinv is None else (lambda v: dinv * v)   # noqa: E731
    c0, ac = scalars(lmin, lmax, iters)
    r = b - A(x)
    nu = np.sqrt(hp.dot(r, r))
    hist = [nu]
    if iters == 0:
        return x, hist
    d = t_(c0) * Minv(r)
    for k in range(iters):
        # iterate k is checked where it left its norm: k = 0 (mod CHECK_EVERY)
        if rtol > 0 and k % CHECK_EVERY == 0 and (hist[k] <= t_(rtol) * nu or hist[k] == 0):
            break
        x = x + d
        r = r - A(d)
        a, c = ac[k]
        d = t_(a) * d + t_(c) * Minv(r)
        hist.append(np.sqrt(hp.dot(r, r)))
    return x, hist
