// BiCGSTAB with right preconditioning (van der Vorst 1992): the short-recurrence local solver of the
// non-symmetric branch, beside the restarted GMRES of gmres.hip.  An extension: the reference offers GMRES only.
//
// Device resident like the CG (cg.hip) and GMRES: all scalars -- rho, alpha, omega, the residual norms, the
// stop decision and the breakdown flag -- live in HBM; every vector kernel folds the per-workgroup partial sums
// of the launch before it in a fixed order (bit-reproducible, no atomics), and once a stop has been decided the
// remaining launches return at once.  The host looks at the state one batch of iterations behind the launches.
//
//   r_0 = b - A x ; rhat = r_0 ; rho_0 = rhat.r_0 ; nu = ||r_0|| ; p_0 = r_0
//   top:   stop if k == max_iters, or ||r_k|| <= rtol nu, or ||r_k|| == 0
//          stop, breakdown 1, if rho_k == 0 or not finite
//   phat = M^-1 p_k ; v = A phat ; sigma = rhat.v
//          stop, breakdown 2, if sigma == 0 or not finite                    (x, r untouched, iters = k)
//   alpha = rho_k / sigma ; s = r_k - alpha v
//   half:  if ||s|| <= rtol nu or ||s|| == 0:  x += alpha phat ; r_{k+1} = s ; iters = k + 1 ; stop
//   shat = M^-1 s ; t = A shat ; tau = t.t ; theta = t.s
//          if tau == 0 or theta == 0 or not finite: the half step as above, stop, breakdown 3
//   omega = theta / tau
//   x += alpha phat + omega shat ; r_{k+1} = s - omega t ; rho_{k+1} = rhat.r_{k+1}
//   beta = (rho_{k+1} / rho_k)(alpha / omega) ; p_{k+1} = r_{k+1} + beta (p_k - omega v)
//
// One iteration: two stop-aware SpMV launches (kSpmvDot, as GMRES uses it) and five vector launches:
//   direction  32 n B (40 n with a stored phat)   top decisions, beta, p, phat = D^-1 p
//   sigma      16 n                               partial sums of rhat.v
//   s          24 - 32 n                          alpha, s, shat = D^-1 s, partial ||s||^2
//   tau/theta  16 n                               two banks of partial sums
//   update     56 - 64 n                          omega, half / breakdown-3 decisions, x, r, partial rhat.r and r.r
// Without a preconditioner phat and shat ARE p and s; for Jacobi in any DiagView form they are stored by the
// direction and s launches; block-Jacobi, ILU(0) and ISAI go through precond_apply between the launches.
// A solve ends with one more direction launch of a single workgroup, which only folds ||r|| and decides.
//
// Who writes what in BicgState, so that no launch reads a value another workgroup of the same launch writes:
//   direction (it = k)  reads rho[(k-1)&1], alpha, omega, r0;  workgroup 0 writes rho[k&1], resn, (r0), stop_iter
//   s                   reads rho[k&1];                        workgroup 0 writes alpha, or stop_iter = k
//   update              reads alpha, r0;                       workgroup 0 writes omega, iters, or stop_iter = k + 1
// Every workgroup takes every decision itself from the folds; a workgroup that sees an early stop_iter = k at its
// entry test leaves like the others would.  The update launch of a half step still has work to do when the stop
// is decided: its stop_iter is k + 1, which the workgroups of launch k read as "not yet".
#include <hip/hip_runtime.h>

#include <climits>

#include "device_utils.hpp"
#include "schwz_hip.h"
#include "schwz_internal.hpp"

namespace schwz {

constexpr int kBicgBatch = SCHWZ_BICGSTAB_POLL_BATCH;  // iterations between two looks of the host at the state

struct BicgState {
    double r0;      // nu = ||b - A x_start||
    double resn;    // the residual norm the last stop test saw (||r||, or ||s|| after a half step)
    double rho[2];  // rho_k in slot k & 1
    double alpha, omega;
    int iters;
    int stop_iter;  // iteration index from which on launches return at once (INT_MAX: not decided)
    int breakdown;  // 0..3
    int pad;
};

// (not isfinite(): the answer must not depend on the floating-point flags of the build)
__device__ __forceinline__ bool bicg_finite(double v)
{
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// Top of iteration `it`: folds rho_it = rhat.r and ||r||^2 (first: both are the ||r_0||^2 of the residual launch),
// takes the top decisions, then p = r + beta (p - omega v) (first: p = r, rhat = r) and phat = D^-1 p where the
// preconditioner is a diagonal.  NTP: non-temporal store of p -- only together with a stored phat: the next
// launch (the SpMV) then reads phat, and p is not read again before the next direction launch, two SpMVs
// later.  Without phat the SpMV reads p itself, and phat is always read by the next launch: plain stores.
template <int U, bool NTP>
__global__ __launch_bounds__(kBlock) void bicg_direction_kernel(int64_t n, double *p, const double *__restrict__ r,
                                                                const double *__restrict__ v, double *__restrict__ phat,
                                                                double *__restrict__ rhat, const DiagView dg,
                                                                const double *rho_partials, const double *rr_partials,
                                                                int nparts, BicgState *st, int it, double rtol,
                                                                int max_iters, int first)
{
    __shared__ double red[4];
    __shared__ double ddict[256];
    if (!first && it >= st->stop_iter) return;
    const double rr = fold_partials(rr_partials, nparts, red);
    const double rho = first ? rr : fold_partials(rho_partials, nparts, red);
    const double resn = sqrt(rr);
    const double nu = first ? resn : st->r0;
    const bool stop = it >= max_iters || resn <= rtol * nu || resn == 0.0;
    const bool bd1 = !stop && (rho == 0.0 || !bicg_finite(rho));
    double beta = 0.0, omega = 0.0;
    if (!first) {
        omega = st->omega;
        beta = (rho / st->rho[(it + 1) & 1]) * (st->alpha / omega);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (first) {
            st->r0 = resn;
            st->iters = 0;
            st->breakdown = 0;
            st->alpha = st->omega = 0.0;
        }
        st->resn = resn;
        st->rho[it & 1] = rho;
        if (bd1) st->breakdown = 1;
        if (stop || bd1)
            st->stop_iter = it;
        else if (first)
            st->stop_iter = INT_MAX;
    }
    if (stop || bd1) return;
    if (dg.mode == 2) {
        if (threadIdx.x < dg.ndict) ddict[threadIdx.x] = dg.dict[threadIdx.x];
        __syncthreads();
    }
    const double *__restrict__ dinv = dg.mode == 1 ? dg.full : nullptr;
    const uint16_t *dc2 = reinterpret_cast<const uint16_t *>(dg.code);
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const vd2 *p2 = reinterpret_cast<const vd2 *>(p);
    const vd2 *r2 = reinterpret_cast<const vd2 *>(r);
    const vd2 *v2 = reinterpret_cast<const vd2 *>(v);
    const vd2 *d2 = reinterpret_cast<const vd2 *>(dinv);
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n2; i0 += stride * U) {
        vd2 pv[U], rv[U], vv[U], dv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                rv[u] = r2[i];
                if (!first) {
                    pv[u] = p2[i];
                    vv[u] = v2[i];
                }
                if (dg.mode) dv[u] = diag_pair(dg, d2, dc2, ddict, i);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                vd2 pn = rv[u];
                if (!first) pn = rv[u] + beta * (pv[u] - omega * vv[u]);
                store2<NTP>(p, i, pn);
                if (dg.mode) store2<false>(phat, i, dv[u] * pn);
                if (first) store2<false>(rhat, i, rv[u]);
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        double pn = r[i];
        if (!first) pn = r[i] + beta * (p[i] - omega * v[i]);
        p[i] = pn;
        if (dg.mode) phat[i] = diag_one(dg, ddict, i) * pn;
        if (first) rhat[i] = r[i];
    }
}

// partial sums of a.b, and with TWO of a.a as well (bank 0: a.a, bank 1: a.b): sigma = rhat.v, and tau = t.t with
// theta = t.s
template <int U, bool TWO>
__global__ __launch_bounds__(kBlock) void bicg_dot_kernel(int64_t n, const double *__restrict__ a,
                                                          const double *__restrict__ b, double *partials_out,
                                                          const BicgState *st, int it)
{
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    double aa = 0.0, ab = 0.0;
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const vd2 *a2 = reinterpret_cast<const vd2 *>(a);
    const vd2 *b2 = reinterpret_cast<const vd2 *>(b);
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n2; i0 += stride * U) {
        vd2 av[U], bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                av[u] = a2[i];
                bv[u] = b2[i];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                if (TWO) {
                    aa += av[u].x * av[u].x;
                    aa += av[u].y * av[u].y;
                }
                ab += av[u].x * bv[u].x;
                ab += av[u].y * bv[u].y;
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        if (TWO) aa += a[i] * a[i];
        ab += a[i] * b[i];
    }
    if (TWO) {
        const double s0 = block_sum(aa, red);
        const double s1 = block_sum(ab, red);
        if (threadIdx.x == 0) {
            partials_out[blockIdx.x] = s0;
            partials_out[gridDim.x + blockIdx.x] = s1;
        }
    } else {
        const double s1 = block_sum(ab, red);
        if (threadIdx.x == 0) partials_out[blockIdx.x] = s1;
    }
}

// alpha = rho / fold(sigma partials), the breakdown-2 decision, s = r - alpha v, shat = D^-1 s where the
// preconditioner is a diagonal, partial sums of ||s||^2.  NTS: non-temporal store of s -- only together with a
// stored shat: the SpMV that follows reads shat, and s waits for the tau/theta launch behind it.  Without shat the
// next launch (the SpMV, or the preconditioner's first kernel) reads s: a plain store.
template <int U, bool NTS>
__global__ __launch_bounds__(kBlock) void bicg_s_kernel(int64_t n, const double *__restrict__ r,
                                                        const double *__restrict__ v, double *__restrict__ s,
                                                        double *__restrict__ shat, const DiagView dg,
                                                        const double *sigma_partials, int nparts, BicgState *st, int it,
                                                        double *partials_out)
{
    __shared__ double red[4];
    __shared__ double ddict[256];
    if (it >= st->stop_iter) return;
    const double sigma = fold_partials(sigma_partials, nparts, red);
    const double alpha = st->rho[it & 1] / sigma;
    // (a quotient that overflows counts as a breakdown too: x never receives a non-finite alpha)
    const bool bd2 = sigma == 0.0 || !bicg_finite(sigma) || !bicg_finite(alpha);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (bd2) {
            st->breakdown = 2;
            st->stop_iter = it;
        } else {
            st->alpha = alpha;
        }
    }
    if (bd2) return;
    if (dg.mode == 2) {
        if (threadIdx.x < dg.ndict) ddict[threadIdx.x] = dg.dict[threadIdx.x];
        __syncthreads();
    }
    const double *__restrict__ dinv = dg.mode == 1 ? dg.full : nullptr;
    const uint16_t *dc2 = reinterpret_cast<const uint16_t *>(dg.code);
    double acc = 0.0;
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const vd2 *r2 = reinterpret_cast<const vd2 *>(r);
    const vd2 *v2 = reinterpret_cast<const vd2 *>(v);
    const vd2 *d2 = reinterpret_cast<const vd2 *>(dinv);
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n2; i0 += stride * U) {
        vd2 rv[U], vv[U], dv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                rv[u] = r2[i];
                vv[u] = v2[i];
                if (dg.mode) dv[u] = diag_pair(dg, d2, dc2, ddict, i);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                const vd2 sv = rv[u] - alpha * vv[u];
                store2<NTS>(s, i, sv);
                if (dg.mode) store2<false>(shat, i, dv[u] * sv);
                acc += sv.x * sv.x;
                acc += sv.y * sv.y;
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double sv = r[i] - alpha * v[i];
        s[i] = sv;
        if (dg.mode) shat[i] = diag_one(dg, ddict, i) * sv;
        acc += sv * sv;
    }
    const double ss = block_sum(acc, red);
    if (threadIdx.x == 0) partials_out[blockIdx.x] = ss;
}

// omega = theta / tau and the half-step and breakdown-3 decisions from the folds, then the full update
// x += alpha phat + omega shat, r = s - omega t with the partial sums of rhat.r and r.r, or the half update
// x += alpha phat, r = s.  x goes out with non-temporal stores: nothing reads it before the update launch of the
// next iteration.  r is read by the direction launch that follows: a plain store.
template <int U>
__global__ __launch_bounds__(kBlock) void bicg_update_kernel(int64_t n, double *__restrict__ x, double *__restrict__ r,
                                                             const double *s, const double *__restrict__ t,
                                                             const double *__restrict__ phat, const double *shat,
                                                             const double *__restrict__ rhat, const double *ss_partials,
                                                             const double *tt_partials, int nparts, BicgState *st,
                                                             int it, double rtol, double *partials_out)
{
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const double sn = sqrt(fold_partials(ss_partials, nparts, red));
    const double tau = fold_partials(tt_partials, nparts, red);
    const double theta = fold_partials(tt_partials + nparts, nparts, red);
    const double alpha = st->alpha;
    const bool half = sn <= rtol * st->r0 || sn == 0.0;
    const double omega = theta / tau;
    const bool bd3 = !half && (tau == 0.0 || theta == 0.0 || !bicg_finite(tau) || !bicg_finite(theta) ||
                               !bicg_finite(omega));
    const bool ends = half || bd3;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->iters = it + 1;
        if (ends) {
            st->resn = sn;
            if (bd3) st->breakdown = 3;
            st->stop_iter = it + 1;  // this launch carries `it`: its other workgroups read "not yet"
        } else {
            st->omega = omega;
        }
    }
    double a0 = 0.0, a1 = 0.0;
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const vd2 *x2 = reinterpret_cast<const vd2 *>(x);
    const vd2 *s2 = reinterpret_cast<const vd2 *>(s);
    const vd2 *t2 = reinterpret_cast<const vd2 *>(t);
    const vd2 *ph2 = reinterpret_cast<const vd2 *>(phat);
    const vd2 *sh2 = reinterpret_cast<const vd2 *>(shat);
    const vd2 *rh2 = reinterpret_cast<const vd2 *>(rhat);
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n2; i0 += stride * U) {
        vd2 xv[U], sv[U], tv[U], pv[U], hv[U], qv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                xv[u] = x2[i];
                sv[u] = s2[i];
                pv[u] = ph2[i];
                if (!ends) {
                    tv[u] = t2[i];
                    hv[u] = sh2[i];
                    qv[u] = rh2[i];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                vd2 xn = xv[u] + alpha * pv[u];
                vd2 rn = sv[u];
                if (!ends) {
                    xn += omega * hv[u];
                    rn -= omega * tv[u];
                    a0 += qv[u].x * rn.x;
                    a0 += qv[u].y * rn.y;
                    a1 += rn.x * rn.x;
                    a1 += rn.y * rn.y;
                }
                store2<true>(x, i, xn);
                store2<false>(r, i, rn);
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        double xn = x[i] + alpha * phat[i];
        double rn = s[i];
        if (!ends) {
            xn += omega * shat[i];
            rn -= omega * t[i];
            a0 += rhat[i] * rn;
            a1 += rn * rn;
        }
        x[i] = xn;
        r[i] = rn;
    }
    if (ends) return;
    const double s0 = block_sum(a0, red);
    const double s1 = block_sum(a1, red);
    if (threadIdx.x == 0) {
        partials_out[blockIdx.x] = s0;
        partials_out[gridDim.x + blockIdx.x] = s1;
    }
}

}  // namespace schwz

using namespace schwz;

struct schwz_bicgstab {
    const schwz_csr *A = nullptr;
    schwz_pcg *pre = nullptr;  // owns the preconditioner (and the SpMV partial-sum banks): adopted, destroyed by hand
    int64_t n = 0;
    bool diag = false;     // Jacobi: phat / shat stored by the direction and s launches
    bool general = false;  // block-Jacobi / ILU / ISAI: precond_apply between the launches
    Dev<double> r, rhat, p, v, s, t;
    Dev<double> phat, shat;  // (unallocated: p and s themselves, without a preconditioner)
    Dev<double> part;        // 6 banks of kMaxGrid: sigma, ||s||^2, tau, theta, rhat.r, r.r
    StateMirror<BicgState> state;
    int variant = 0;
};

namespace schwz {

// the solver around a preconditioner object it takes over (destroyed with it); when this fails `pre` stays the
// caller's
int bicgstab_create_adopt(const schwz_csr *A, schwz_pcg *pre, schwz_bicgstab **out)
{
    schwz_bicgstab *s = new schwz_bicgstab();
    s->A = A;
    s->n = A->v.nrows;
    s->pre = pre;
    s->diag = pre->precond == SCHWZ_PRECOND_JACOBI && pre->diag.mode != 0;
    s->general = pre->precond != SCHWZ_PRECOND_NONE && !s->diag;
    const size_t ld = (size_t)((s->n + 1) & ~int64_t(1));  // whole 16-byte elements
    int rc = SCHWZ_OK;
    for (Dev<double> *vec : {&s->r, &s->rhat, &s->p, &s->v, &s->s, &s->t})
        if (!rc) rc = vec->alloc(ld);
    if (!rc && (s->diag || s->general) && !(rc = s->phat.alloc(ld))) rc = s->shat.alloc(ld);
    if (!rc && !(rc = s->part.alloc(6 * kMaxGrid))) rc = s->state.create();
    if (rc) {
        (void)hipGetLastError();
        s->pre = nullptr;
        schwz_bicgstab_destroy(s);
        return rc;
    }
    *out = s;
    return SCHWZ_OK;
}

schwz_pcg *bicgstab_precond(schwz_bicgstab *s) { return s->pre; }

// schwz_ras_restart: the state of the last solve (what schwz_bicgstab_last_stats and schwz_bicgstab_breakdown report)
// back to zeros, as created
int bicgstab_forget(schwz_bicgstab *s, hipStream_t st) { return s ? s->state.reset(st) : SCHWZ_OK; }

schwz_pcg *bicgstab_release_precond(schwz_bicgstab *s)
{
    schwz_pcg *pre = s->pre;
    s->pre = nullptr;
    return pre;
}

}  // namespace schwz

extern "C" {

int schwz_bicgstab_create(const schwz_csr *A, int precond, int block_size, int par_ilu_sweeps, int trisolve_sweeps,
                          schwz_bicgstab **out)
{
    int rc = pcg_check_ilu_sweeps(precond, par_ilu_sweeps, trisolve_sweeps);
    if (rc) return rc;
    SCHWZ_REQUIRE(A && out, "schwz_bicgstab_create: null argument");
    SCHWZ_REQUIRE(A->v.nrows == A->v.ncols, "schwz_bicgstab_create: matrix must be square");
    schwz_pcg *pre = nullptr;
    rc = par_ilu_sweeps || trisolve_sweeps ? pcg_create_impl(A, precond, block_size, par_ilu_sweeps, trisolve_sweeps, &pre)
                                           : schwz_pcg_create_ex(A, precond, block_size, &pre);
    if (rc) return rc;
    if ((rc = bicgstab_create_adopt(A, pre, out))) schwz_pcg_destroy(pre);
    return rc;
}

void schwz_bicgstab_destroy(schwz_bicgstab *s)
{
    if (!s) return;
    schwz_pcg_destroy(s->pre);
    delete s;
}

int schwz_bicgstab_last_stats(schwz_bicgstab *s, int *h_iters, double *h_resnorm)
{
    SCHWZ_REQUIRE(s && h_iters && h_resnorm, "schwz_bicgstab_last_stats: null argument");
    if (const int rc = s->state.read_blocking()) return rc;
    *h_iters = s->state.host(0).iters;
    *h_resnorm = s->state.host(0).resn;
    return SCHWZ_OK;
}

int schwz_bicgstab_breakdown(schwz_bicgstab *s)
{
    if (!s) return 0;
    if (s->state.read_blocking()) {
        set_error("schwz_bicgstab_breakdown: the state could not be read");
        return -1;
    }
    return s->state.host(0).breakdown;
}

#define BICG_LAUNCH(kernel_u1, kernel_u2, grid, ...)                                           \
    do {                                                                                       \
        if (wide)                                                                              \
            hipLaunchKernelGGL(kernel_u2, dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);       \
        else                                                                                   \
            hipLaunchKernelGGL(kernel_u1, dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);       \
    } while (0)

int schwz_bicgstab_solve(schwz_bicgstab *s, const double *d_b, double *d_x, double rtol, int max_iters, int *h_iters,
                         double *h_resnorm, schwz_stream stream)
{
    SCHWZ_REQUIRE(s && d_b && d_x, "schwz_bicgstab_solve: null argument");
    SCHWZ_REQUIRE(max_iters >= 0, "schwz_bicgstab_solve: negative max_iters");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = s->n;
    if (n == 0) {
        if (h_iters) *h_iters = 0;
        if (h_resnorm) *h_resnorm = 0.0;
        return SCHWZ_OK;
    }
    const CsrView &A = s->A->v;
    // one lane per 16-byte element (two rows), like the CG's vector kernels: the grid is capped, and the kernels
    // stride with two elements in flight per lane, above 2048 * 256 elements = 1 048 576 rows
    const int gs = spmv_grid(A, s->variant), gv = grid_for((n + 1) / 2);
    const bool wide = (n >> 1) > (int64_t)gv * kBlock;
    double *sig = s->part, *ssq = s->part + kMaxGrid, *tt = s->part + 2 * kMaxGrid, *rho = s->part + 4 * kMaxGrid;
    double *phat = s->phat ? s->phat : s->p, *shat = s->shat ? s->shat : s->s;
    const DiagView dg = s->diag ? s->pre->diag : DiagView();
    int rc;
    // ---- r = b - A x, ||r||^2 ----
    SpmvArgs a;
    a.x = d_x;
    a.b = d_b;
    a.y = s->r;
    a.p = s->p;  // the kernel also writes p := r, which the first direction launch repeats (with rhat and phat)
    a.partials = s->pre->partials;
    a.stream_part = s->pre->stream_part;
    if ((rc = launch_spmv(A, kSpmvResidInit, a, s->variant, st))) return rc;
    bool stopped = false;
    s->state.begin();
    for (int k = 0; !stopped; ++k) {
        const int first = k == 0 ? 1 : 0;
        const bool closing = k >= max_iters;  // folds ||r|| and decides: one workgroup, which stores no vector
        const double *rho_in = first ? s->pre->partials + gs : rho;
        const double *rr_in = first ? s->pre->partials + gs : rho + gv;
        const int nparts = first ? gs : gv;
        if (s->diag)
            BICG_LAUNCH((bicg_direction_kernel<1, true>), (bicg_direction_kernel<2, true>), closing ? 1 : gv, n, s->p,
                        s->r, s->v, s->phat, s->rhat, dg, rho_in, rr_in, nparts, s->state.dev(), k, rtol, max_iters, first);
        else
            BICG_LAUNCH((bicg_direction_kernel<1, false>), (bicg_direction_kernel<2, false>), closing ? 1 : gv, n, s->p,
                        s->r, s->v, (double *)nullptr, s->rhat, dg, rho_in, rr_in, nparts, s->state.dev(), k, rtol, max_iters,
                        first);
        if (closing) break;
        if (s->general && (rc = precond_apply(s->pre, s->p, s->phat, st))) return rc;
        SpmvArgs q;
        q.x = phat;
        q.y = s->v;
        q.partials = s->pre->partials;  // phat . v, unused
        q.stream_part = s->pre->stream_part;
        q.stop_iter = &s->state.dev()->stop_iter;
        q.it = k;
        if ((rc = launch_spmv(A, kSpmvDot, q, s->variant, st))) return rc;
        BICG_LAUNCH((bicg_dot_kernel<1, false>), (bicg_dot_kernel<2, false>), gv, n, s->rhat, s->v, sig, s->state.dev(), k);
        if (s->diag)
            BICG_LAUNCH((bicg_s_kernel<1, true>), (bicg_s_kernel<2, true>), gv, n, s->r, s->v, s->s, s->shat, dg, sig, gv,
                        s->state.dev(), k, ssq);
        else
            BICG_LAUNCH((bicg_s_kernel<1, false>), (bicg_s_kernel<2, false>), gv, n, s->r, s->v, s->s,
                        (double *)nullptr, dg, sig, gv, s->state.dev(), k, ssq);
        // (speculative when the half step ends the solve: nothing reads shat and t then)
        if (s->general && (rc = precond_apply(s->pre, s->s, s->shat, st))) return rc;
        q.x = shat;
        q.y = s->t;
        if ((rc = launch_spmv(A, kSpmvDot, q, s->variant, st))) return rc;
        BICG_LAUNCH((bicg_dot_kernel<1, true>), (bicg_dot_kernel<2, true>), gv, n, s->t, s->s, tt, s->state.dev(), k);
        BICG_LAUNCH((bicg_update_kernel<1>), (bicg_update_kernel<2>), gv, n, d_x, s->r, s->s, s->t, phat, shat, s->rhat,
                    ssq, tt, gv, s->state.dev(), k, rtol, rho);
        SCHWZ_HIP_TRY(hipGetLastError());
        if ((k + 1) % kBicgBatch != 0 || k + 1 >= max_iters) continue;
        // the host reads the state one batch behind the launches
        if ((rc = s->state.poll(st, &stopped))) return rc;
    }
    SCHWZ_HIP_TRY(hipGetLastError());
    if (h_iters || h_resnorm) {
        if ((rc = s->state.read(st))) return rc;
        if (h_iters) *h_iters = s->state.host(0).iters;
        if (h_resnorm) *h_resnorm = s->state.host(0).resn;
    }
    return SCHWZ_OK;
}

}  // extern "C"
