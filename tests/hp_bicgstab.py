"""Extended-precision reference of the device-resident BiCGSTAB (csrc/bicgstab.hip), built on hp_reference: the
statement of the algorithm the solver documents, line for line, in `np.longdouble` or (the same text) in float64.

    r_0 = b - A x ;  rhat = r_0 ;  rho_0 = rhat.r_0 ;  nu = ||r_0|| ;  p_0 = r_0
    for k = 0, 1, ...
      top:   stop if k == max_iters, or ||r_k|| <= rtol nu, or ||r_k|| == 0
             stop, breakdown = 1, if rho_k == 0 or rho_k is not finite
      phat = M^-1 p_k ;  v = A phat ;  sigma = rhat.v
             stop, breakdown = 2, if sigma == 0 or sigma is not finite          (x, r untouched, iters = k)
      alpha = rho_k / sigma ;  s = r_k - alpha v
      half:  if ||s|| <= rtol nu or ||s|| == 0:  x += alpha phat ; r_{k+1} = s ; iters = k+1 ; stop
      shat = M^-1 s ;  t = A shat ;  tau = t.t ;  theta = t.s
             if tau == 0 or theta == 0 or either is not finite:
                 x += alpha phat ; r_{k+1} = s ; iters = k+1 ; stop, breakdown = 3
      omega = theta / tau
      x += alpha phat + omega shat ;  r_{k+1} = s - omega t ;  rho_{k+1} = rhat.r_{k+1}
      beta = (rho_{k+1}/rho_k)(alpha/omega) ;  p_{k+1} = r_{k+1} + beta (p_k - omega v)
"""
import numpy as np

import hp_reference as hp

LD = hp.LD


def bicgstab(rp, col, val, b, x0, precond_apply, iters, rtol=0.0, dtype=LD):
    """Right-preconditioned BiCGSTAB (van der Vorst 1992), at most `iters` iterations.

    Returns (x, hist, half_hist, breakdown): hist[k] = ||r_k|| from the recurrence (hist[0] the start residual
    norm; after a half-step stop the last entry is ||s||), len(hist) - 1 the iteration count; half_hist[k] = ||s||
    of iteration k, for every iteration that formed s; breakdown 0..3."""
    hp._guard(dtype)
    t_ = np.dtype(dtype).type
    A = lambda w: hp.spmv(rp, col, val, w, dtype)   # noqa: E731
    b = np.asarray(b, dtype=dtype)
    x = np.array(x0, dtype=dtype) if x0 is not None else np.zeros(len(b), dtype=dtype)
    r = b - A(x)
    rhat = r.copy()
    rho = hp.dot(rhat, r)
    nu = np.sqrt(hp.dot(r, r))
    p = r.copy()
    hist, half_hist, breakdown = [nu], [], 0
    rn = nu
    k = 0
    while True:
        if k == iters or rn <= t_(rtol) * nu or rn == 0:
            break
        if rho == 0 or not np.isfinite(rho):
            breakdown = 1
            break
        phat = precond_apply(p)
        v = A(phat)
        sigma = hp.dot(rhat, v)
        if sigma == 0 or not np.isfinite(sigma):
            breakdown = 2
            break
        alpha = rho / sigma
        s = r - alpha * v
        sn = np.sqrt(hp.dot(s, s))
        half_hist.append(sn)
        if sn <= t_(rtol) * nu or sn == 0:
            x = x + alpha * phat
            r = s
            hist.append(sn)
            k += 1
            break
        shat = precond_apply(s)
        t = A(shat)
        tau = hp.dot(t, t)
        theta = hp.dot(t, s)
        if tau == 0 or theta == 0 or not np.isfinite(tau) or not np.isfinite(theta):
            x = x + alpha * phat
            r = s
            hist.append(sn)
            k += 1
            breakdown = 3
            break
        omega = theta / tau
        x = x + (alpha * phat + omega * shat)
        r = s - omega * t
        rho_new = hp.dot(rhat, r)
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        rho = rho_new
        rn = np.sqrt(hp.dot(r, r))
        hist.append(rn)
        k += 1
    return x, hist, half_hist, breakdown
