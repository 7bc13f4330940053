// Chebyshev local solve (schwz_cheb): the Jacobi-preconditioned Chebyshev iteration for SPD matrices, one
// reduction-free launch per iteration.  An extension: the reference's symmetric local solver is CG only.
//
// For SPD A, with M = I or M = diag(A), the spectrum of M^-1 A assumed in [lmin, lmax]:
//   theta = (lmax + lmin) / 2 ; delta = (lmax - lmin) / 2 ; sigma = theta / delta
//
//   r_0 = b - A x_0 ;  rho_0 = 1 / sigma ;  d_0 = (1 / theta) M^-1 r_0
//   for k = 0 ... m-1:
//       x_{k+1} = x_k + d_k
//       r_{k+1} = r_k - A d_k
//       rho_{k+1} = 1 / (2 sigma - rho_k)
//       d_{k+1} = (rho_{k+1} rho_k) d_k + (2 rho_{k+1} / delta) M^-1 r_{k+1}
//
// max_iters = m is the number of corrections applied, the polynomial degree.  The scalars depend on the bounds and on
// k alone: the host computes them in fp64, in exactly the order written above, and passes them to the launches by
// value.  There is no inner product in the iteration, so there are no partial-sum banks to fold, no state struct to
// read and ONE launch per iteration: launch k (k >= 1) gathers d_{k-1}, and at its own row i
//   q_i = (A d)_i ;  r_i -= q_i ;  x_i += d_i ;  d'_i = a d_i + c dinv_i r_i   (d' stored to the other d buffer)
// d ping-pongs because the launch gathers d from neighbouring rows while it produces d'; x and r are touched at the
// lane's own row only and are updated in place.  Launch 0 (START) gathers x: r = b - A x, d_0 = (1/theta) dinv r.
//
// Fixed work (rtol <= 0): START, m - 1 iteration launches, one vector launch x += d_{m-1}: m matrix passes, no host
// poll, no device state read.  ||r_m|| is computed only when somebody asks (h_resnorm, *_last_stats): one NORM-only
// launch of ||r_{m-1} - A d_{m-1}||, which stores nothing but its partial sums.
// With a tolerance: the launches that produce r_k for k = 0 (mod SCHWZ_CHEB_CHECK_EVERY) and for k = m also write one
// fp64 partial sum of r_i^2 per workgroup, and every workgroup of the NEXT launch folds them itself in a fixed order
// (fold_partials, as cg_f32.hip has it: no fence, no atomic, no ticket counter) and returns at once when
// ||r_k|| <= rtol ||r_0|| or the norm is zero; workgroup 0 records the stop in ChebState for the launches behind it
// and for the host, which polls one chunk behind as schwz_pcg_f32_solve does.
//
// The solver reads plain CSR, whatever coding the upload chose: on stencil matrices the fp64 z-sweep walk of CG moves
// far fewer matrix bytes; there this solver is opt-in and expected to be slower per pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "schwz_internal.hpp"
#include "device_utils.hpp"
#include "stream_pipeline.hpp"

namespace schwz {

constexpr int kChebSeq = 3;  // consecutive tiles per short-lived workgroup (spmv_stream.hip), more where the grid is capped

struct ChebState {
    double nu2;  // ||r_0||^2
    double rr;   // ||r_iters||^2
    int iters;
    int stop_iter;  // INT_MAX while the solve runs
};

enum ChebForm {
    kChebStart = 0,     // r = b - A x ; d' = c dinv r ; x untouched
    kChebIter = 1,      // r -= A d ; x += d ; d' = a d + c dinv r
    kChebNormOnly = 2,  // partial sums of ||b - A g||^2, nothing else stored
};

struct ChebArgs {
    const double *g = nullptr;     // the gathered vector: d_{k-1}, or x (START)
    const double *b = nullptr;     // START: the right-hand side; NORM-only: the vector A g is subtracted from
    double *r = nullptr;           // residual, updated in place at the lane's own row
    double *x = nullptr;           // iterate, updated in place at the lane's own row
    double *dn = nullptr;          // d' (never the gathered buffer)
    const double *dinv = nullptr;  // 1 / diag(A); null: M = I
    double a = 0.0, c = 0.0;
    double *part = nullptr;        // NORM forms: one partial sum of r_i^2 per workgroup
    // with a tolerance only (st != null)
    ChebState *st = nullptr;
    const double *chk = nullptr;   // the partial sums of ||r_{k-1}||^2 where k - 1 is a checked iterate
    int nchk = 0;
    int k = 0;                     // the iterate this launch produces
    double rtol = 0.0;
    int seq = kChebSeq;
};

// Start of a launch of a solve with a tolerance; true: the workgroup leaves (uniform over the workgroup).
// Launch k leaves when an earlier launch recorded a stop before k, or when iterate k - 1 was checked and passes.
// Workgroup 0 records; workgroups that read stop_iter while it is being written see INT_MAX or k - 1 and decide the
// same either way.
__device__ __forceinline__ bool cheb_leaves(const ChebArgs &a, double *red)
{
    if (!a.st) return false;
    if (a.st->stop_iter < a.k) return true;
    if (!a.chk) return false;
    const double rr = fold_partials(a.chk, a.nchk, red);
    const double nu2 = a.k == 1 ? rr : a.st->nu2;
    const bool stop = sqrt(rr) <= a.rtol * sqrt(nu2) || rr == 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (a.k == 1) a.st->nu2 = rr;
        if (stop) {
            a.st->rr = rr;
            a.st->iters = a.k - 1;
            a.st->stop_iter = a.k - 1;
        }
    }
    return stop;
}

// The tile pipeline of stream_pipeline.hpp, short-lived workgroups of `seq` consecutive tiles, with the iteration's
// row update as its epilogue.  The one branch in the tile loop is the one around the stores: a lane past the tile's
// last row repeats that row's loads and arithmetic and stores nothing, because r and x are updated in place (a second
// store of the same value would be harmless, a second load after another wave's store would not).
template <int FORM, bool NORM, int CAP>
__global__ __launch_bounds__(kBlock) void cheb_stream_kernel(CsrView A, ChebArgs a)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    if (FORM == kChebIter && cheb_leaves(a, red)) return;
    const int tid = threadIdx.x;
    if (FORM == kChebStart && a.st && blockIdx.x == 0 && tid == 0) {
        a.st->nu2 = 0.0;
        a.st->rr = 0.0;
        a.st->iters = 0;
        a.st->stop_iter = INT_MAX;
    }
    double acc = 0.0;
    const double *const own = FORM == kChebIter ? (const double *)a.r : a.b;  // what A g is subtracted from
    const double *const dinv = a.dinv ? a.dinv : own;  // a valid address either way (the value is selected away)
    struct Ops {
        double o0, o1, o2, o3;  // own, dinv, d, x at the lane's row
    };
    auto load = [&](int rowc) -> Ops {
        Ops o{own[rowc], 0.0, 0.0, 0.0};
        if (FORM != kChebNormOnly) o.o1 = dinv[rowc];
        if (FORM == kChebIter) {
            o.o2 = a.g[rowc];
            o.o3 = a.x[rowc];
        }
        return o;
    };
    auto row = [&](double sum, const Ops &o, int rowc, bool mine) {
        const double rn = o.o0 - sum;
        if (FORM != kChebNormOnly) {
            const double z = a.dinv ? o.o1 * rn : rn;
            const double cz = a.c * z;
            const double dnew = FORM == kChebIter ? a.a * o.o2 + cz : cz;
            const double xn = o.o3 + o.o2;
            if (mine) {
                a.r[rowc] = rn;
                a.dn[rowc] = dnew;
                if (FORM == kChebIter) a.x[rowc] = xn;
            }
        }
        if (NORM) {
            const double t = rn * rn;
            acc += mine ? t : 0.0;
        }
    };
    SCHWZ_STREAM_PIPELINE(A, CAP, double, A.val, a.g, a.seq, false, Ops, load, row)
    if (NORM) {
        const double s0 = block_sum(acc, red);
        if (tid == 0) a.part[blockIdx.x] = s0;
    }
}

// Every other matrix (a row longer than the largest CAP, a tile that does not fit the aligned window): one row per
// lane, summed in CSR order, grid-stride, the same epilogues.  Built for correctness only.
template <int FORM, bool NORM>
__global__ __launch_bounds__(kBlock) void cheb_rows_kernel(CsrView A, ChebArgs a)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    if (FORM == kChebIter && cheb_leaves(a, red)) return;
    if (FORM == kChebStart && a.st && blockIdx.x == 0 && threadIdx.x == 0) {
        a.st->nu2 = 0.0;
        a.st->rr = 0.0;
        a.st->iters = 0;
        a.st->stop_iter = INT_MAX;
    }
    const double *const own = FORM == kChebIter ? (const double *)a.r : a.b;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.nrows; i += stride) {
        double sum = 0.0;
        for (int j = A.rp[i]; j < A.rp[i + 1]; ++j) {
            const double pv = A.val[j] * a.g[A.col[j]];
            sum += pv;
        }
        const double rn = own[i] - sum;
        if (FORM != kChebNormOnly) {
            const double z = a.dinv ? a.dinv[i] * rn : rn;
            const double cz = a.c * z;
            if (FORM == kChebIter) {
                const double di = a.g[i];
                a.x[i] = a.x[i] + di;
                a.dn[i] = a.a * di + cz;
            } else {
                a.dn[i] = cz;
            }
            a.r[i] = rn;
        }
        if (NORM) acc += rn * rn;
    }
    if (NORM) {
        const double s0 = block_sum(acc, red);
        if (threadIdx.x == 0) a.part[blockIdx.x] = s0;
    }
}

// x += d: the last correction of a fixed-work solve
__global__ __launch_bounds__(kBlock) void cheb_axpy_kernel(int64_t n, double *__restrict__ x, const double *__restrict__ d)
{
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) x[i] = x[i] + d[i];
}

// End of a solve with a tolerance (one workgroup): no stop so far, so iterate m stands; its norm from the partial sums
__global__ __launch_bounds__(kBlock) void cheb_finish_kernel(ChebState *st, const double *part, int nparts, int m)
{
    __shared__ double red[4];
    if (st->stop_iter != INT_MAX) return;
    const double rr = fold_partials(part, nparts, red);
    if (threadIdx.x == 0) {
        st->rr = rr;
        st->iters = m;
        st->stop_iter = m;
    }
}

// The lazy norm of a fixed-work solve (one workgroup): the partial sums of the NORM-only launch folded into the state
__global__ __launch_bounds__(kBlock) void cheb_fold_kernel(ChebState *st, const double *part, int nparts)
{
    __shared__ double red[4];
    const double rr = fold_partials(part, nparts, red);
    if (threadIdx.x == 0) st->rr = rr;
}

// Gershgorin bound on M^-1 A: max_i |dinv_i| sum_j |a_ij|, the row sum in CSR order; the maximum over rows is
// order-independent, hence deterministic (a NaN sticks).  With dinv != null: dinv_i = 1 / a_ii, and the smallest row
// whose diagonal is missing, zero, negative or not finite in pbad (LLONG_MAX: none).  One slot per workgroup.
__global__ __launch_bounds__(kBlock) void cheb_bound_kernel(CsrView A, double *__restrict__ dinv, double *__restrict__ pmax,
                                                            long long *__restrict__ pbad)
{
#pragma clang fp contract(off)
    __shared__ double smax[4];
    __shared__ long long sbad[4];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double m = 0.0;
    long long bad = LLONG_MAX;
    auto take = [](double cur, double v) -> double { return (v > cur || v != v) ? v : cur; };
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.nrows; i += stride) {
        double s = 0.0, dg = 0.0;
        bool has = false;
        for (int j = A.rp[i]; j < A.rp[i + 1]; ++j) {
            const double v = A.val[j];
            s += fabs(v);
            if (A.col[j] == i) {
                dg = v;
                has = true;
            }
        }
        double di = 1.0;
        if (dinv) {
            if (!has || !(dg > 0.0) || !isfinite(dg))
                bad = min(bad, (long long)i);
            else
                di = 1.0 / dg;
            dinv[i] = di;
        }
        m = take(m, fabs(di) * s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m = take(m, __shfl_down(m, off, 64));
        bad = min(bad, (long long)__shfl_down(bad, off, 64));
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        smax[w] = m;
        sbad[w] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        pmax[blockIdx.x] = take(take(smax[0], smax[1]), take(smax[2], smax[3]));
        pbad[blockIdx.x] = min(min(sbad[0], sbad[1]), min(sbad[2], sbad[3]));
    }
}

}  // namespace schwz

using namespace schwz;

struct schwz_cheb {
    const schwz_csr *A = nullptr;
    int precond = 0;
    int64_t n = 0;
    double lmin = 0.0, lmax = 0.0;
    Dev<double> r, d[2], dinv;
    Dev<double> part;  // 2 banks of kMaxGrid partial sums: the NORM launches alternate
    StateMirror<ChebState> state;
    bool stream_ok = false;  // the tile pipeline takes the matrix
    int gs = 0, gv = 0;      // grids of the matrix launches and of the vector launch, both <= kMaxGrid
    int seq = kChebSeq;
    // the last solve
    bool fixed = false;      // fixed work: iters and norm are the host's (last_iters, last_rr), not the state's
    int last_iters = 0;
    bool norm_pending = false;  // fixed work: ||r_m|| not computed yet
    int norm_d = 0;             // ... from r and d[norm_d]
    double last_rr = 0.0;       // ||r_m||^2 once computed (NaN: never computable, max_iters = 0 and nobody asked)
};

// schwz_ras_restart: what the object remembers of its last solve is forgotten, as created -- the pending norm is
// DROPPED (it would be the norm of a residual of the old right-hand side), the counters and the device state are zero
int schwz::cheb_forget(schwz_cheb *s, hipStream_t st)
{
    if (!s) return SCHWZ_OK;
    s->fixed = false;
    s->last_iters = 0;
    s->norm_pending = false;
    s->norm_d = 0;
    s->last_rr = 0.0;
    return s->state.reset(st);
}

template <int FORM, bool NORM>
static void cheb_launch_form(const schwz_cheb *s, const ChebArgs &a, hipStream_t st)
{
    const CsrView &A = s->A->v;
    if (s->stream_ok) {
        stream_cap_dispatch(A, [&](auto cap) {
            hipLaunchKernelGGL((cheb_stream_kernel<FORM, NORM, decltype(cap)::value>), dim3(s->gs), dim3(kBlock), 0, st, A, a);
        });
    } else {
        hipLaunchKernelGGL((cheb_rows_kernel<FORM, NORM>), dim3(s->gs), dim3(kBlock), 0, st, A, a);
    }
}

static void cheb_launch(const schwz_cheb *s, int form, bool norm, const ChebArgs &a, hipStream_t st)
{
    if (form == kChebStart) {
        if (norm)
            cheb_launch_form<kChebStart, true>(s, a, st);
        else
            cheb_launch_form<kChebStart, false>(s, a, st);
    } else if (form == kChebIter) {
        if (norm)
            cheb_launch_form<kChebIter, true>(s, a, st);
        else
            cheb_launch_form<kChebIter, false>(s, a, st);
    } else {
        cheb_launch_form<kChebNormOnly, true>(s, a, st);
    }
}

static int cheb_build(schwz_cheb *s)
{
    const CsrView &A = s->A->v;
    const int64_t n = s->n;
    // Every grid holds at most kMaxGrid workgroups, so that the workgroups of the next launch can fold its partial
    // sums themselves.  Row-per-lane kernels (fallback, vector launch, bound): one row per lane up to
    // kBlock * kMaxGrid = 524 288 rows, grid-stride beyond.  Tile pipeline: short-lived workgroups of kChebSeq
    // consecutive tiles while such a grid fits (6144 tiles, about 1.5 M rows), longer runs of tiles beyond.
    s->gv = grid_for(n);
    s->stream_ok = stream_takes(A);
    if (s->stream_ok) {
        const int nslots = stream_slots(A);
        const int per_xcd = kMaxGrid / kXcds;
        s->seq = std::max(kChebSeq, (nslots + per_xcd - 1) / per_xcd);
        s->gs = kXcds * std::max(1, (nslots + s->seq - 1) / s->seq);
    } else {
        s->gs = grid_for(n);
    }
    int rc;
    for (Dev<double> *v : {&s->r, &s->d[0], &s->d[1]})
        if ((rc = v->alloc((size_t)n, true))) return rc;
    if ((rc = s->part.alloc((size_t)2 * kMaxGrid, true)) || (rc = s->state.create())) return rc;
    if (s->precond == SCHWZ_PRECOND_JACOBI && (rc = s->dinv.alloc((size_t)n, true))) return rc;
    if (n == 0) {
        s->lmax = 1.0;
        s->lmin = s->lmax / 30.0;
        return SCHWZ_OK;
    }
    // the bound (and 1 / diag): one slot per workgroup, the maximum taken here
    const int g = s->gv;
    Dev<long long> d_bad;
    if ((rc = d_bad.alloc((size_t)g))) return rc;
    std::vector<double> h_max((size_t)g);
    std::vector<long long> h_bad((size_t)g);
    hipLaunchKernelGGL(cheb_bound_kernel, dim3(g), dim3(kBlock), 0, 0, A, s->dinv, s->part, d_bad);
    SCHWZ_HIP_TRY(hipGetLastError());
    SCHWZ_HIP_TRY(hipMemcpy(h_max.data(), s->part, (size_t)g * sizeof(double), hipMemcpyDeviceToHost));
    SCHWZ_HIP_TRY(hipMemcpy(h_bad.data(), d_bad, (size_t)g * sizeof(long long), hipMemcpyDeviceToHost));
    long long bad = LLONG_MAX;
    double lmax = 0.0;
    for (int i = 0; i < g; ++i) {
        bad = std::min(bad, h_bad[(size_t)i]);
        const double v = h_max[(size_t)i];
        lmax = (v > lmax || v != v) ? v : lmax;
    }
    if (bad != LLONG_MAX) {
        char msg[200];
        std::snprintf(msg, sizeof(msg),
                      "schwz_cheb_create: row %lld has no positive finite diagonal entry (Jacobi needs one)", bad);
        set_error(msg);
        return SCHWZ_ERR_NOT_SPD;
    }
    if (!(lmax > 0.0) || !std::isfinite(lmax)) {
        set_error("schwz_cheb_create: the Gershgorin bound of the matrix is not a positive finite number");
        return SCHWZ_ERR_NOT_SPD;
    }
    s->lmax = lmax;
    s->lmin = lmax / 30.0;
    SCHWZ_HIP_TRY(hipDeviceSynchronize());
    return SCHWZ_OK;
}

// ||b - A g|| of a fixed-work solve, by one NORM-only launch on `st`; synchronises `st`
static int cheb_norm_now(schwz_cheb *s, const double *own, const double *g, hipStream_t st)
{
    ChebArgs a;
    a.g = g;
    a.b = own;
    a.part = s->part;
    a.seq = s->seq;
    cheb_launch(s, kChebNormOnly, true, a, st);
    hipLaunchKernelGGL(cheb_fold_kernel, dim3(1), dim3(kBlock), 0, st, s->state.dev(), (const double *)s->part, s->gs);
    SCHWZ_HIP_TRY(hipGetLastError());
    if (const int rc = s->state.read(st)) return rc;
    s->last_rr = s->state.host(0).rr;
    s->norm_pending = false;
    return SCHWZ_OK;
}

extern "C" {

int schwz_cheb_create(const schwz_csr *A, int precond, schwz_cheb **out)
{
    // the argument checks come before the matrix is looked at (they need no device)
    SCHWZ_REQUIRE(out, "schwz_cheb_create: null output");
    *out = nullptr;
    SCHWZ_REQUIRE(precond >= SCHWZ_PRECOND_NONE && precond <= SCHWZ_PRECOND_ISAI,
                  "schwz_cheb_create: unknown preconditioner");
    if (precond != SCHWZ_PRECOND_NONE && precond != SCHWZ_PRECOND_JACOBI) {
        set_error("schwz_cheb_create: the Chebyshev local solve exists without a preconditioner and with scalar Jacobi only");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    SCHWZ_REQUIRE(A, "schwz_cheb_create: null matrix");
    SCHWZ_REQUIRE(A->v.nrows == A->v.ncols, "schwz_cheb_create: matrix not square");
    schwz_cheb *s = new schwz_cheb();
    s->A = A;
    s->precond = precond;
    s->n = A->v.nrows;
    const int rc = cheb_build(s);
    if (rc) {
        schwz_cheb_destroy(s);
        return rc;
    }
    *out = s;
    return SCHWZ_OK;
}

void schwz_cheb_destroy(schwz_cheb *s) { delete s; }

int schwz_cheb_bounds(const schwz_cheb *s, double *lmin, double *lmax)
{
    SCHWZ_REQUIRE(s && lmin && lmax, "schwz_cheb_bounds: null argument");
    *lmin = s->lmin;
    *lmax = s->lmax;
    return SCHWZ_OK;
}

int schwz_cheb_set_bounds(schwz_cheb *s, double lmin, double lmax)
{
    // (the values are checked first: they need no solver)
    SCHWZ_REQUIRE(std::isfinite(lmin) && std::isfinite(lmax) && lmin > 0.0 && lmin < lmax,
                  "schwz_cheb_set_bounds: the bounds must be finite with 0 < lmin < lmax");
    SCHWZ_REQUIRE(s, "schwz_cheb_set_bounds: null solver");
    s->lmin = lmin;
    s->lmax = lmax;
    return SCHWZ_OK;
}

int schwz_cheb_solve(schwz_cheb *s, const double *d_b, double *d_x, double rtol, int max_iters, int *h_iters,
                     double *h_resnorm, schwz_stream stream)
{
    SCHWZ_REQUIRE(s && d_b && d_x, "schwz_cheb_solve: null argument");
    SCHWZ_REQUIRE(max_iters >= 0, "schwz_cheb_solve: negative max_iters");
    hipStream_t st = (hipStream_t)stream;
    const int m = max_iters;
    s->fixed = true;
    s->last_iters = 0;
    s->norm_pending = false;
    s->last_rr = 0.0;
    if (s->n == 0) {
        if (h_iters) *h_iters = 0;
        if (h_resnorm) *h_resnorm = 0.0;
        return SCHWZ_OK;
    }
    if (m == 0) {
        // nothing is launched and x keeps its bits; the norm of b - A x only for a caller that asks now
        s->last_rr = std::numeric_limits<double>::quiet_NaN();
        if (h_resnorm) {
            const int rc = cheb_norm_now(s, d_b, d_x, st);
            if (rc) return rc;
            *h_resnorm = std::sqrt(s->last_rr);
        }
        if (h_iters) *h_iters = 0;
        return SCHWZ_OK;
    }
    // the scalars, in fp64 and in the order of the header
    const double theta = (s->lmax + s->lmin) / 2.0;
    const double delta = (s->lmax - s->lmin) / 2.0;
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    const bool tol = rtol > 0.0;
    ChebArgs a;
    a.dinv = s->dinv;
    a.r = s->r;
    a.x = d_x;
    a.seq = s->seq;
    a.rtol = rtol;
    a.st = tol ? s->state.dev() : nullptr;
    a.nchk = s->gs;
    // START: r_0 = b - A x_0, d_0 = (1 / theta) M^-1 r_0
    int cur = 0;
    a.g = d_x;
    a.b = d_b;
    a.dn = s->d[0];
    a.c = 1.0 / theta;
    a.k = 0;
    a.part = s->part;
    cheb_launch(s, kChebStart, tol, a, st);
    SCHWZ_HIP_TRY(hipGetLastError());
    auto advance = [&]() {  // the scalars of the launch that produces d_{k+1} from d_k
        const double rho_next = 1.0 / (2.0 * sigma - rho);
        a.a = rho_next * rho;
        a.c = 2.0 * rho_next / delta;
        rho = rho_next;
    };
    if (!tol) {
        for (int k = 1; k < m; ++k) {
            advance();
            a.g = s->d[cur];
            a.dn = s->d[cur ^ 1];
            a.k = k;
            cheb_launch(s, kChebIter, false, a, st);
            cur ^= 1;
        }
        hipLaunchKernelGGL(cheb_axpy_kernel, dim3(s->gv), dim3(kBlock), 0, st, s->n, d_x, (const double *)s->d[cur]);
        SCHWZ_HIP_TRY(hipGetLastError());
        s->last_iters = m;
        s->norm_pending = true;
        s->norm_d = cur;
        if (h_resnorm) {
            const int rc = cheb_norm_now(s, s->r, s->d[cur], st);  // on the asking call's stream
            if (rc) return rc;
            *h_resnorm = std::sqrt(s->last_rr);
        }
        if (h_iters) *h_iters = m;
        return SCHWZ_OK;
    }
    // With a tolerance: launch k = 1 ... m produces iterate k; it checks iterate k - 1 where that one left its norm,
    // and leaves its own where k = 0 (mod SCHWZ_CHEB_CHECK_EVERY) or k = m.  The host control flow is that of
    // schwz_pcg_f32_solve: growing chunks of launches (ChunkSchedule) and a poll of the pinned state copy one chunk
    // behind; launches past the stop return at once.
    s->fixed = false;
    ChunkSchedule chunks;
    int k = 1, nb = 0, rc;
    bool prev_norm = true, stopped = false;
    s->state.begin();
    while (k <= m && !stopped) {
        const int end = chunks.end(k - 1, m, true);
        for (; k <= end; ++k) {
            advance();
            const bool norm = (k % SCHWZ_CHEB_CHECK_EVERY) == 0 || k == m;
            a.g = s->d[cur];
            a.dn = s->d[cur ^ 1];
            a.k = k;
            a.chk = prev_norm ? s->part + (size_t)nb * kMaxGrid : nullptr;
            a.part = s->part + (size_t)(nb ^ 1) * kMaxGrid;
            cheb_launch(s, kChebIter, norm, a, st);
            if (norm) nb ^= 1;
            prev_norm = norm;
            cur ^= 1;
        }
        SCHWZ_HIP_TRY(hipGetLastError());
        if (k <= m) {
            if ((rc = s->state.poll(st, &stopped))) return rc;
            chunks.grow();
        }
    }
    // (after a stop the host may have ended between two norm launches: the finish kernel then leaves at once)
    hipLaunchKernelGGL(cheb_finish_kernel, dim3(1), dim3(kBlock), 0, st, s->state.dev(),
                       (const double *)(s->part + (size_t)nb * kMaxGrid), s->gs, m);
    SCHWZ_HIP_TRY(hipGetLastError());
    if (h_iters || h_resnorm) {
        if ((rc = s->state.read(st))) return rc;
        if (h_iters) *h_iters = s->state.host(0).iters;
        if (h_resnorm) *h_resnorm = std::sqrt(s->state.host(0).rr);
    }
    return SCHWZ_OK;
}

int schwz_cheb_last_stats(schwz_cheb *s, int *h_iters, double *h_resnorm)
{
    SCHWZ_REQUIRE(s && h_iters && h_resnorm, "schwz_cheb_last_stats: null argument");
    if (s->fixed) {
        // the lazy norm runs behind a device synchronisation, on the null stream: never on a saved stream handle
        SCHWZ_HIP_TRY(hipDeviceSynchronize());
        if (s->norm_pending) {
            const int rc = cheb_norm_now(s, s->r, s->d[s->norm_d], nullptr);
            if (rc) return rc;
        }
        *h_iters = s->last_iters;
        *h_resnorm = std::sqrt(s->last_rr);
        return SCHWZ_OK;
    }
    if (const int rc = s->state.read_blocking()) return rc;
    *h_iters = s->state.host(0).iters;
    *h_resnorm = std::sqrt(s->state.host(0).rr);
    return SCHWZ_OK;
}

}  // extern "C"
