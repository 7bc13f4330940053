// Restarted GMRES(m) with right preconditioning: the local solver of the non-symmetric branch of
// Solve::setup_local_solver / Solve::local_solve (source/solve.cpp:486-520, 750-753;
// gko::solver::Gmres with krylov_dim = settings.restart_iter and the Combined(Iteration,
// ResidualNormReduction) criterion of solve.cpp:469-479).  Ginkgo's source is not part of the
// reference checkout: the algorithm is Saad & Schultz (1986) with modified Gram-Schmidt and Givens
// rotations, the same restatement as oracle/schwz_oracle.c::schwz_or_gmres, which scipy's GMRES
// reproduces iteration for iteration.
//
// Device resident like the CG (cg.hip): all scalars -- the Hessenberg column, the rotations,
// the rotated right-hand side, the stop decision -- live in HBM; every vector kernel folds the
// per-workgroup partial sums of the launch before it in a fixed order (bit-reproducible, no
// atomics), and once the tolerance test has fired the remaining launches of the cycle return at
// once.  The host looks at the 32-byte state one cycle behind the launches.
//
// Per Krylov vector j: z = M^-1 v_j, w = A z, j + 1 projection passes
// (w -= h_i v_i fused with the next dot), one normalisation pass.  Vector traffic grows with j;
// the SpMV and the preconditioner are the kernels of the CG path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "device_utils.hpp"
#include "schwz_hip.h"
#include "schwz_internal.hpp"

namespace schwz {

struct GmresState {
    double r0;      // ||b - A x_start||, the reference of the reduction test
    double resn;    // current residual norm (true at a cycle start, rotated rhs inside a cycle)
    int stop_iter;  // Krylov vectors after which the solve stops (INT_MAX: not decided)
    int iters;      // Krylov vectors built so far
};

static int gm_grid(int64_t n)
{
    int64_t g = (n + kBlock - 1) / kBlock;
    if (g > kMaxGrid) g = kMaxGrid;
    return g < 1 ? 1 : (int)g;
}

// after the residual SpMV of a cycle start: beta, the stop tests of the loop top, g = beta e_1
__global__ void gmres_start_kernel(GmresState *st, const double *rr_partials, int nparts, double rtol, int it_base,
                                   int first, int max_iters, double *g, int m)
{
    __shared__ double red[4];
    if (!first && it_base >= st->stop_iter) return;
    const double beta = sqrt(fold_partials(rr_partials, nparts, red));
    if (threadIdx.x == 0) {
        if (first) {
            st->r0 = beta;
            st->iters = 0;
            st->stop_iter = INT_MAX;
        }
        st->resn = beta;
        if (it_base >= max_iters || beta <= rtol * st->r0 || beta == 0.0) st->stop_iter = it_base;
        g[0] = beta;
        for (int i = 1; i <= m; ++i) g[i] = 0.0;
    }
}

// v_0 = r / beta (in place)
__global__ __launch_bounds__(kBlock) void gmres_scale_kernel(int64_t n, double *__restrict__ v, const GmresState *st,
                                                             int it_base)
{
    if (it_base >= st->stop_iter) return;
    const double beta = st->resn;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) v[i] /= beta;
}

// One projection pass of modified Gram-Schmidt.  With `vprev`: h = fold(partials_in) is the
// coefficient against vprev (stored by workgroup 0), w -= h vprev.  Then the partial sums of
// w . vnext (vnext == nullptr: of w . w) for the next pass.
__global__ __launch_bounds__(kBlock) void gmres_project_kernel(int64_t n, double *__restrict__ w,
                                                               const double *__restrict__ vprev,
                                                               const double *__restrict__ vnext,
                                                               const double *partials_in, int nparts,
                                                               double *partials_out, double *h_out,
                                                               const GmresState *st, int it)
{
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    double h = 0.0;
    if (vprev) {
        h = fold_partials(partials_in, nparts, red);
        if (blockIdx.x == 0 && threadIdx.x == 0) *h_out = h;
    }
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double wv = w[i];
        if (vprev) {
            wv -= h * vprev[i];
            w[i] = wv;
        }
        acc += wv * (vnext ? vnext[i] : wv);
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials_out[blockIdx.x] = s;
}

// v_{j+1} = w / ||w||; workgroup 0 finishes column j of the Hessenberg matrix: the old rotations,
// the new one, the rotated right-hand side and the stop test.
__global__ __launch_bounds__(kBlock) void gmres_finish_kernel(int64_t n, const double *__restrict__ w,
                                                              double *__restrict__ vnext, const double *ww_partials,
                                                              int nparts, double *H, double *cs, double *sn, double *g,
                                                              int m, int j, GmresState *st, int it, double rtol)
{
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const double hn = sqrt(fold_partials(ww_partials, nparts, red));
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        vnext[i] = hn != 0.0 ? w[i] / hn : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double *h = H + (size_t)j * (size_t)(m + 1);
        h[j + 1] = hn;
        for (int i = 0; i < j; ++i) {
            const double t = cs[i] * h[i] + sn[i] * h[i + 1];
            h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1];
            h[i] = t;
        }
        double c = 1.0, s = 0.0;
        if (h[j + 1] != 0.0) {
            const double rr = hypot(h[j], h[j + 1]);
            c = h[j] / rr;
            s = h[j + 1] / rr;
        }
        cs[j] = c;
        sn[j] = s;
        h[j] = c * h[j] + s * h[j + 1];
        h[j + 1] = 0.0;
        g[j + 1] = -s * g[j];
        g[j] = c * g[j];
        const double resn = fabs(g[j + 1]);
        st->resn = resn;
        st->iters = it + 1;
        // other workgroups of this launch compare `it` with stop_iter concurrently: it only ever
        // drops to it + 1, which they read as "not yet"
        if (resn <= rtol * st->r0) st->stop_iter = it + 1;
    }
}

// End of a cycle that built k = min(launched, stop_iter - it_base) vectors: H y = g by back
// substitution (every workgroup, redundantly: k is small), t = sum_i y_i v_i.
__global__ __launch_bounds__(kBlock) void gmres_combine_kernel(int64_t n, const double *__restrict__ V, int64_t ldv,
                                                               double *__restrict__ t, const double *H,
                                                               const double *g, int m, int launched,
                                                               const GmresState *st, int it_base)
{
    extern __shared__ double y[];  // m
    if (it_base >= st->stop_iter) return;
    const int k = min(launched, st->stop_iter - it_base);
    if (threadIdx.x == 0) {
        for (int i = k - 1; i >= 0; --i) {
            double s = g[i];
            for (int q = i + 1; q < k; ++q) s -= H[i + (size_t)q * (size_t)(m + 1)] * y[q];
            y[i] = s / H[i + (size_t)i * (size_t)(m + 1)];
        }
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double s = 0.0;
        for (int q = 0; q < k; ++q) s += y[q] * V[(size_t)q * (size_t)ldv + (size_t)i];
        t[i] = s;
    }
}

// x += z
__global__ __launch_bounds__(kBlock) void gmres_axpy_kernel(int64_t n, double *__restrict__ x,
                                                            const double *__restrict__ z, const GmresState *st,
                                                            int it_base)
{
    if (it_base >= st->stop_iter) return;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) x[i] += z[i];
}

// ---------------------------------------------------------------------------------------------------------------
// Compressed-basis GMRES (SCHWZ_GMRES_BASIS_F32): the Krylov basis is stored in fp32, all arithmetic stays fp64, and
// the orthogonalisation is blocked classical Gram-Schmidt applied twice (CGS2) in three passes whatever j is:
//   A  h  = V^T w                                  (cb_dot_kernel, cb_fold_kernel)
//   B  w -= V h, then h' = V^T w in the same launch (cb_sub_dot_kernel, cb_fold_kernel): a lane re-reads only rows
//      it wrote itself, so the second round of dot products needs no launch of its own
//   C  w -= V h', partial sums of ||w||^2          (cb_sub_norm_kernel)
//   finish: H(0..j, j) = h + h', H(j+1, j) = ||w||, v_{j+1} = fl32(w / ||w||) stored as fp32 AND widened back to
//      fp64 in `vw`, the vector the preconditioner and the SpMV of the next step read: the Arnoldi relation holds
//      for the stored basis.
// A lane works on four consecutive rows (one 16-byte load per fp32 column, two per fp64 vector); the basis is taken in
// groups of kCbGroup columns, whose accumulators stay in registers, and w is re-read once per group.  Partial sums:
// one fp64 value per (column, workgroup).  They are folded by a launch of their own with one workgroup per
// coefficient, which writes h to HBM where the next pass reads it uniformly: were every workgroup of the next pass
// to fold all (j + 1) x grid partial sums itself, as the one-scalar solvers do, each would read 0.25 MB at m = 30.
// The pass grids are capped at kCbMaxGrid workgroups (four per CU), which halves that fold and the finish kernel's.
// ---------------------------------------------------------------------------------------------------------------

constexpr int kCbGroup = 8;
constexpr int kCbMaxGrid = 1024;
constexpr int kCbRows = 4;  // rows per lane and step

typedef float vf4 __attribute__((ext_vector_type(4)));

static int cb_grid(int64_t n)
{
    int64_t g = (n + (int64_t)kBlock * kCbRows - 1) / ((int64_t)kBlock * kCbRows);
    if (g > kCbMaxGrid) g = kCbMaxGrid;
    return g < 1 ? 1 : (int)g;
}

// rows r .. r + 3 of an fp64 vector / an fp32 column (r a multiple of 4: 16-byte aligned); rows past n read as zero
__device__ __forceinline__ void cb_load(const double *w, int64_t r, int64_t n, double (&x)[kCbRows])
{
    if (r + kCbRows <= n) {
        const vd2 a = reinterpret_cast<const vd2 *>(w + r)[0], b = reinterpret_cast<const vd2 *>(w + r)[1];
        x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y;
    } else {
#pragma unroll
        for (int k = 0; k < kCbRows; ++k) x[k] = r + k < n ? w[r + k] : 0.0;
    }
}

__device__ __forceinline__ void cb_load(const float *v, int64_t r, int64_t n, double (&x)[kCbRows])
{
    if (r + kCbRows <= n) {
        const vf4 a = *reinterpret_cast<const vf4 *>(v + r);
        x[0] = (double)a.x, x[1] = (double)a.y, x[2] = (double)a.z, x[3] = (double)a.w;
    } else {
#pragma unroll
        for (int k = 0; k < kCbRows; ++k) x[k] = r + k < n ? (double)v[r + k] : 0.0;
    }
}

__device__ __forceinline__ void cb_store(double *w, int64_t r, int64_t n, const double (&x)[kCbRows])
{
    if (r + kCbRows <= n) {
        vd2 a, b;
        a.x = x[0], a.y = x[1], b.x = x[2], b.y = x[3];
        reinterpret_cast<vd2 *>(w + r)[0] = a;
        reinterpret_cast<vd2 *>(w + r)[1] = b;
    } else {
#pragma unroll
        for (int k = 0; k < kCbRows; ++k)
            if (r + k < n) w[r + k] = x[k];
    }
}

__device__ __forceinline__ void cb_store(float *v, int64_t r, int64_t n, const double (&x)[kCbRows])
{
    if (r + kCbRows <= n) {
        vf4 a;
        a.x = (float)x[0], a.y = (float)x[1], a.z = (float)x[2], a.w = (float)x[3];
        *reinterpret_cast<vf4 *>(v + r) = a;
    } else {
#pragma unroll
        for (int k = 0; k < kCbRows; ++k)
            if (r + k < n) v[r + k] = (float)x[k];
    }
}

// part[c * gridDim.x + blockIdx.x] = this workgroup's share of w . v_c for the nv columns of V, a group at a time.
// `red`: 4 * kCbGroup doubles.
__device__ __forceinline__ void cb_dots(int64_t n, const double *w, const float *V, int64_t ldv, int nv, double *part,
                                        double *red)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock * kCbRows;
    for (int g0 = 0; g0 < nv; g0 += kCbGroup) {
        const int cnt = min(kCbGroup, nv - g0);
        const float *Vg = V + (size_t)g0 * (size_t)ldv;
        double acc[kCbGroup];
#pragma unroll
        for (int k = 0; k < kCbGroup; ++k) acc[k] = 0.0;
        for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCbRows; r < n; r += stride) {
            double wv[kCbRows];
            cb_load(w, r, n, wv);
#pragma unroll
            for (int k = 0; k < kCbGroup; ++k) {
                if (k < cnt) {
                    double v[kCbRows];
                    cb_load(Vg + (size_t)k * (size_t)ldv, r, n, v);
#pragma unroll
                    for (int e = 0; e < kCbRows; ++e) acc[k] += wv[e] * v[e];
                }
            }
        }
        block_sum_lds<kCbGroup>(acc, red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < kCbGroup; ++k)
                if (k < cnt) part[(size_t)(g0 + k) * gridDim.x + blockIdx.x] = acc[k];
        }
    }
}

// w -= sum_c h_c v_c on the lane's rows; with NORM the lane's share of ||w||^2 afterwards
template <bool NORM>
__device__ __forceinline__ double cb_subtract(int64_t n, double *w, const float *V, int64_t ldv, int nv, const double *h)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock * kCbRows;
    double ww = 0.0;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCbRows; r < n; r += stride) {
        double wv[kCbRows];
        cb_load(w, r, n, wv);
        for (int g0 = 0; g0 < nv; g0 += kCbGroup) {
            const int cnt = min(kCbGroup, nv - g0);
            double v[kCbGroup][kCbRows];
#pragma unroll
            for (int k = 0; k < kCbGroup; ++k)
                if (k < cnt) cb_load(V + (size_t)(g0 + k) * (size_t)ldv, r, n, v[k]);
#pragma unroll
            for (int k = 0; k < kCbGroup; ++k) {
                if (k < cnt) {
                    const double hc = h[g0 + k];
#pragma unroll
                    for (int e = 0; e < kCbRows; ++e) wv[e] -= hc * v[k][e];
                }
            }
        }
        cb_store(w, r, n, wv);
        if (NORM) {
#pragma unroll
            for (int e = 0; e < kCbRows; ++e) ww += wv[e] * wv[e];
        }
    }
    return ww;
}

// v_0 = fl32(r / beta): the fp32 column and, in place over r, its widened copy
__global__ __launch_bounds__(kBlock) void cb_scale_kernel(int64_t n, double *__restrict__ vw, float *__restrict__ v0,
                                                          const GmresState *st, int it_base)
{
    if (it_base >= st->stop_iter) return;
    const double beta = st->resn;
    const int64_t stride = (int64_t)gridDim.x * kBlock * kCbRows;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCbRows; r < n; r += stride) {
        double x[kCbRows];
        cb_load(vw, r, n, x);
#pragma unroll
        for (int e = 0; e < kCbRows; ++e) x[e] = (double)(float)(x[e] / beta);
        cb_store(v0, r, n, x);
        cb_store(vw, r, n, x);
    }
}

// pass A
__global__ __launch_bounds__(kBlock) void cb_dot_kernel(int64_t n, const double *__restrict__ w,
                                                        const float *__restrict__ V, int64_t ldv, int nv,
                                                        double *__restrict__ part, const GmresState *st, int it)
{
    __shared__ double red[4 * kCbGroup];
    if (it >= st->stop_iter) return;
    cb_dots(n, w, V, ldv, nv, part, red);
}

// one workgroup per coefficient: h_c = the fold of its gridDim-of-the-pass partial sums, in a fixed order
__global__ __launch_bounds__(kBlock) void cb_fold_kernel(const double *__restrict__ part, int nparts,
                                                         double *__restrict__ h, const GmresState *st, int it)
{
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const double s = fold_partials(part + (size_t)blockIdx.x * (size_t)nparts, nparts, red);
    if (threadIdx.x == 0) h[blockIdx.x] = s;
}

// pass B (w is read and written through one pointer: the dot products re-read what this lane stored)
__global__ __launch_bounds__(kBlock) void cb_sub_dot_kernel(int64_t n, double *w, const float *__restrict__ V,
                                                            int64_t ldv, int nv, const double *__restrict__ h,
                                                            double *__restrict__ part, const GmresState *st, int it)
{
    __shared__ double red[4 * kCbGroup];
    if (it >= st->stop_iter) return;
    (void)cb_subtract<false>(n, w, V, ldv, nv, h);
    cb_dots(n, w, V, ldv, nv, part, red);
}

// pass C
__global__ __launch_bounds__(kBlock) void cb_sub_norm_kernel(int64_t n, double *__restrict__ w,
                                                             const float *__restrict__ V, int64_t ldv, int nv,
                                                             const double *__restrict__ h, double *__restrict__ ww_part,
                                                             const GmresState *st, int it)
{
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const double s = block_sum(cb_subtract<true>(n, w, V, ldv, nv, h), red);
    if (threadIdx.x == 0) ww_part[blockIdx.x] = s;
}

// gmres_finish_kernel for the compressed basis: v_{j+1} = fl32(w / ||w||) as fp32 column and as widened copy;
// workgroup 0 sets column j of H to h + h' and then does exactly what gmres_finish_kernel does with it.
__global__ __launch_bounds__(kBlock) void cb_finish_kernel(int64_t n, const double *__restrict__ w,
                                                           float *__restrict__ vnext, double *__restrict__ vw,
                                                           const double *ww_partials, int nparts, const double *h1,
                                                           const double *h2, double *H, double *cs, double *sn,
                                                           double *g, int m, int j, GmresState *st, int it, double rtol)
{
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const double hn = sqrt(fold_partials(ww_partials, nparts, red));
    const int64_t stride = (int64_t)gridDim.x * kBlock * kCbRows;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCbRows; r < n; r += stride) {
        double x[kCbRows];
        cb_load(w, r, n, x);
#pragma unroll
        for (int e = 0; e < kCbRows; ++e) x[e] = hn != 0.0 ? (double)(float)(x[e] / hn) : 0.0;
        cb_store(vnext, r, n, x);
        cb_store(vw, r, n, x);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double *h = H + (size_t)j * (size_t)(m + 1);
        for (int i = 0; i <= j; ++i) h[i] = h1[i] + h2[i];
        h[j + 1] = hn;
        for (int i = 0; i < j; ++i) {
            const double t = cs[i] * h[i] + sn[i] * h[i + 1];
            h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1];
            h[i] = t;
        }
        double c = 1.0, s = 0.0;
        if (h[j + 1] != 0.0) {
            const double rr = hypot(h[j], h[j + 1]);
            c = h[j] / rr;
            s = h[j + 1] / rr;
        }
        cs[j] = c;
        sn[j] = s;
        h[j] = c * h[j] + s * h[j + 1];
        h[j + 1] = 0.0;
        g[j + 1] = -s * g[j];
        g[j] = c * g[j];
        const double resn = fabs(g[j + 1]);
        st->resn = resn;
        st->iters = it + 1;
        // (see gmres_finish_kernel: stop_iter only ever drops to it + 1)
        if (resn <= rtol * st->r0) st->stop_iter = it + 1;
    }
}

// gmres_combine_kernel reading the fp32 basis
__global__ __launch_bounds__(kBlock) void cb_combine_kernel(int64_t n, const float *__restrict__ V, int64_t ldv,
                                                            double *__restrict__ t, const double *H, const double *g,
                                                            int m, int launched, const GmresState *st, int it_base)
{
    extern __shared__ double y[];  // m
    if (it_base >= st->stop_iter) return;
    const int k = min(launched, st->stop_iter - it_base);
    if (threadIdx.x == 0) {
        for (int i = k - 1; i >= 0; --i) {
            double s = g[i];
            for (int q = i + 1; q < k; ++q) s -= H[i + (size_t)q * (size_t)(m + 1)] * y[q];
            y[i] = s / H[i + (size_t)i * (size_t)(m + 1)];
        }
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock * kCbRows;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCbRows; r < n; r += stride) {
        double s[kCbRows] = {0.0, 0.0, 0.0, 0.0};
        for (int q = 0; q < k; ++q) {
            double v[kCbRows];
            cb_load(V + (size_t)q * (size_t)ldv, r, n, v);
#pragma unroll
            for (int e = 0; e < kCbRows; ++e) s[e] += y[q] * v[e];
        }
        cb_store(t, r, n, s);
    }
}

}  // namespace schwz

using namespace schwz;

struct schwz_gmres {
    const schwz_csr *A = nullptr;
    schwz_pcg *pre = nullptr;  // owns the preconditioner (and the SpMV partial-sum banks): adopted, destroyed by hand
    int64_t n = 0, ldv = 0;
    int m = 1;
    Dev<double> V;  // (m + 1) vectors of ldv
    Dev<double> w, z;
    Dev<double> H, cs, sn, g;
    Dev<double> part;  // 2 banks of kMaxGrid
    StateMirror<GmresState> state;
    int variant = 0;
    // compressed basis (SCHWZ_GMRES_BASIS_F32): V stays empty
    int basis = SCHWZ_GMRES_BASIS_F64;
    int64_t ldvf = 0;
    Dev<float> Vf;            // (m + 1) fp32 columns of ldvf
    Dev<double> vw;           // the current basis vector widened back to fp64
    Dev<double> h1, h2;       // m coefficients each: the two rounds of CGS2
    Dev<double> cbpart;       // (m + 1) banks of cb_grid(n) partial sums: m for the dot products, one for ||w||^2
};

namespace schwz {

// the solver around a preconditioner object it takes over (destroyed with it); when this fails `pre` stays the
// caller's
int gmres_create_adopt(const schwz_csr *A, int restart, int basis, schwz_pcg *pre, schwz_gmres **out)
{
    schwz_gmres *s = new schwz_gmres();
    s->A = A;
    s->n = A->v.nrows;
    s->m = restart;
    s->basis = basis;
    s->ldv = (s->n + 1) & ~int64_t(1);   // 16-byte aligned columns
    s->ldvf = (s->n + 3) & ~int64_t(3);  // ... of fp32; w, z and vw are as long, so that four rows load at once
    s->pre = pre;
    const bool cb = basis == SCHWZ_GMRES_BASIS_F32;
    const size_t ld = cb ? (size_t)(s->ldvf ? s->ldvf : 4) : (size_t)(s->ldv ? s->ldv : 2), m = (size_t)restart;
    int rc;
    if ((rc = cb ? s->Vf.alloc(ld * (m + 1)) : s->V.alloc(ld * (m + 1))) || (rc = s->w.alloc(ld)) ||
        (rc = s->z.alloc(ld)) ||
        (cb && ((rc = s->vw.alloc(ld)) || (rc = s->h1.alloc(m)) || (rc = s->h2.alloc(m)) ||
                (rc = s->cbpart.alloc((m + 1) * (size_t)cb_grid(s->n))))) ||
        (rc = s->H.alloc((m + 1) * m, true)) || (rc = s->cs.alloc(m)) || (rc = s->sn.alloc(m)) ||
        (rc = s->g.alloc(m + 1)) || (rc = s->part.alloc(2 * kMaxGrid)) || (rc = s->state.create())) {
        s->pre = nullptr;
        schwz_gmres_destroy(s);
        return rc;
    }
    *out = s;
    return SCHWZ_OK;
}

schwz_pcg *gmres_precond(schwz_gmres *s) { return s->pre; }

// schwz_ras_restart: the state of the last solve (what schwz_gmres_last_stats reports) back to zeros, as created
int gmres_forget(schwz_gmres *s, hipStream_t st) { return s ? s->state.reset(st) : SCHWZ_OK; }

int gmres_basis(const schwz_gmres *s) { return s->basis; }

schwz_pcg *gmres_release_precond(schwz_gmres *s)
{
    schwz_pcg *pre = s->pre;
    s->pre = nullptr;
    return pre;
}

}  // namespace schwz

extern "C" {

int schwz_gmres_create(const schwz_csr *A, int precond, int block_size, int restart, schwz_gmres **out)
{
    return schwz_gmres_create_ex(A, precond, block_size, restart, 0, 0, out);
}

int schwz_gmres_create_ex(const schwz_csr *A, int precond, int block_size, int restart, int par_ilu_sweeps,
                          int trisolve_sweeps, schwz_gmres **out)
{
    return schwz_gmres_create_basis(A, precond, block_size, restart, par_ilu_sweeps, trisolve_sweeps,
                                    SCHWZ_GMRES_BASIS_F64, out);
}

int schwz_gmres_create_basis(const schwz_csr *A, int precond, int block_size, int restart, int par_ilu_sweeps,
                             int trisolve_sweeps, int basis, schwz_gmres **out)
{
    SCHWZ_REQUIRE(basis == SCHWZ_GMRES_BASIS_F64 || basis == SCHWZ_GMRES_BASIS_F32,
                  "schwz_gmres_create_basis: unknown basis type");
    int rc = pcg_check_ilu_sweeps(precond, par_ilu_sweeps, trisolve_sweeps);
    if (rc) return rc;
    SCHWZ_REQUIRE(A && out, "schwz_gmres_create: null argument");
    SCHWZ_REQUIRE(A->v.nrows == A->v.ncols, "schwz_gmres_create: matrix must be square");
    SCHWZ_REQUIRE(restart >= 1, "schwz_gmres_create: restart (krylov_dim) must be >= 1");
    SCHWZ_REQUIRE(restart <= 2048, "schwz_gmres_create: restart above 2048 is not supported");
    schwz_pcg *pre = nullptr;
    rc = par_ilu_sweeps || trisolve_sweeps
             ? pcg_create_impl(A, precond, block_size, par_ilu_sweeps, trisolve_sweeps, &pre)
             : schwz_pcg_create_ex(A, precond, block_size, &pre);
    if (rc) return rc;
    if ((rc = gmres_create_adopt(A, restart, basis, pre, out))) schwz_pcg_destroy(pre);
    return rc;
}

void schwz_gmres_destroy(schwz_gmres *s)
{
    if (!s) return;
    schwz_pcg_destroy(s->pre);
    delete s;
}

int schwz_gmres_last_stats(schwz_gmres *s, int *h_iters, double *h_resnorm)
{
    SCHWZ_REQUIRE(s && h_iters && h_resnorm, "schwz_gmres_last_stats: null argument");
    if (const int rc = s->state.read_blocking()) return rc;
    *h_iters = s->state.host(0).iters;
    *h_resnorm = s->state.host(0).resn;
    return SCHWZ_OK;
}

int schwz_gmres_basis(const schwz_gmres *s) { return s ? s->basis : SCHWZ_GMRES_BASIS_F64; }

// the solve with the compressed basis: the cycle of schwz_gmres_solve with the three-pass orthogonalisation
static int gmres_solve_cb(schwz_gmres *s, const double *d_b, double *d_x, double rtol, int max_iters, int *h_iters,
                          double *h_resnorm, hipStream_t st)
{
    const int64_t n = s->n, ldv = s->ldvf;
    const CsrView &A = s->A->v;
    const int m = s->m;
    const int gs = spmv_grid(A, s->variant), gv = gm_grid(n), gc = cb_grid(n);
    double *ww_part = s->cbpart + (size_t)m * (size_t)gc;
    bool stopped = false;
    s->state.begin();
    for (int c = 0; !stopped; ++c) {
        const int it_base = c * m;
        // ---- r = b - A x in fp64 -> beta, loop-top tests, v_0 = fl32(r / beta) ----
        SpmvArgs a;
        a.x = d_x;
        a.b = d_b;
        a.y = s->vw;
        a.p = s->w;  // the kernel also writes p := r; w is scratch here
        a.partials = s->pre->partials;
        a.stream_part = s->pre->stream_part;
        int rc = launch_spmv(A, kSpmvResidInit, a, s->variant, st);
        if (rc) return rc;
        hipLaunchKernelGGL(gmres_start_kernel, dim3(1), dim3(kBlock), 0, st, s->state.dev(), s->pre->partials + gs, gs, rtol,
                           it_base, c == 0 ? 1 : 0, max_iters, s->g, m);
        hipLaunchKernelGGL(cb_scale_kernel, dim3(gc), dim3(kBlock), 0, st, n, s->vw, s->Vf, s->state.dev(), it_base);
        const int launched = std::min(m, max_iters - it_base);
        for (int j = 0; j < launched; ++j) {
            const int it = it_base + j, nv = j + 1;
            if ((rc = precond_apply(s->pre, s->vw, s->z, st))) return rc;
            SpmvArgs q;
            q.x = s->z;
            q.y = s->w;
            q.partials = s->pre->partials;  // z . w, unused
            q.stream_part = s->pre->stream_part;
            q.stop_iter = &s->state.dev()->stop_iter;
            q.it = it;
            if ((rc = launch_spmv(A, kSpmvDot, q, s->variant, st))) return rc;
            hipLaunchKernelGGL(cb_dot_kernel, dim3(gc), dim3(kBlock), 0, st, n, s->w, s->Vf, ldv, nv, s->cbpart,
                               s->state.dev(), it);
            hipLaunchKernelGGL(cb_fold_kernel, dim3(nv), dim3(kBlock), 0, st, s->cbpart, gc, s->h1, s->state.dev(), it);
            hipLaunchKernelGGL(cb_sub_dot_kernel, dim3(gc), dim3(kBlock), 0, st, n, s->w, s->Vf, ldv, nv, s->h1,
                               s->cbpart, s->state.dev(), it);
            hipLaunchKernelGGL(cb_fold_kernel, dim3(nv), dim3(kBlock), 0, st, s->cbpart, gc, s->h2, s->state.dev(), it);
            hipLaunchKernelGGL(cb_sub_norm_kernel, dim3(gc), dim3(kBlock), 0, st, n, s->w, s->Vf, ldv, nv, s->h2, ww_part,
                               s->state.dev(), it);
            hipLaunchKernelGGL(cb_finish_kernel, dim3(gc), dim3(kBlock), 0, st, n, s->w,
                               s->Vf + (size_t)(j + 1) * (size_t)ldv, s->vw, ww_part, gc, s->h1, s->h2, s->H, s->cs, s->sn,
                               s->g, m, j, s->state.dev(), it, rtol);
        }
        // ---- x += M^-1 (V y) ----
        hipLaunchKernelGGL(cb_combine_kernel, dim3(gc), dim3(kBlock), sizeof(double) * (size_t)m, st, n, s->Vf, ldv, s->w,
                           s->H, s->g, m, launched, s->state.dev(), it_base);
        if ((rc = precond_apply(s->pre, s->w, s->z, st))) return rc;
        hipLaunchKernelGGL(gmres_axpy_kernel, dim3(gv), dim3(kBlock), 0, st, n, d_x, s->z, s->state.dev(), it_base);
        SCHWZ_HIP_TRY(hipGetLastError());
        if (it_base + launched >= max_iters) break;
        // the host reads the state one cycle behind the launches
        if ((rc = s->state.poll(st, &stopped))) return rc;
    }
    if (h_iters || h_resnorm) {
        if (const int rc = s->state.read(st)) return rc;
        if (h_iters) *h_iters = s->state.host(0).iters;
        if (h_resnorm) *h_resnorm = s->state.host(0).resn;
    }
    return SCHWZ_OK;
}

int schwz_gmres_solve(schwz_gmres *s, const double *d_b, double *d_x, double rtol, int max_iters, int *h_iters,
                      double *h_resnorm, schwz_stream stream)
{
    SCHWZ_REQUIRE(s && d_b && d_x, "schwz_gmres_solve: null argument");
    SCHWZ_REQUIRE(max_iters >= 0, "schwz_gmres_solve: negative max_iters");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = s->n;
    if (n == 0) {
        if (h_iters) *h_iters = 0;
        if (h_resnorm) *h_resnorm = 0.0;
        return SCHWZ_OK;
    }
    if (s->basis == SCHWZ_GMRES_BASIS_F32) return gmres_solve_cb(s, d_b, d_x, rtol, max_iters, h_iters, h_resnorm, st);
    const CsrView &A = s->A->v;
    const int m = s->m;
    const int gs = spmv_grid(A, s->variant), gv = gm_grid(n);
    double *bank[2] = {s->part, s->part + kMaxGrid};
    bool stopped = false;
    s->state.begin();
    for (int c = 0; !stopped; ++c) {
        const int it_base = c * m;
        // ---- r = b - A x -> v_0, beta, loop-top tests ----
        SpmvArgs a;
        a.x = d_x;
        a.b = d_b;
        a.y = s->V;
        a.p = s->w;  // the kernel also writes p := r; w is scratch here
        a.partials = s->pre->partials;
        a.stream_part = s->pre->stream_part;
        int rc = launch_spmv(A, kSpmvResidInit, a, s->variant, st);
        if (rc) return rc;
        hipLaunchKernelGGL(gmres_start_kernel, dim3(1), dim3(kBlock), 0, st, s->state.dev(), s->pre->partials + gs, gs, rtol,
                           it_base, c == 0 ? 1 : 0, max_iters, s->g, m);
        hipLaunchKernelGGL(gmres_scale_kernel, dim3(gv), dim3(kBlock), 0, st, n, s->V, s->state.dev(), it_base);
        const int launched = std::min(m, max_iters - it_base);
        for (int j = 0; j < launched; ++j) {
            const int it = it_base + j;
            double *vj = s->V + (size_t)j * (size_t)s->ldv;
            if ((rc = precond_apply(s->pre, vj, s->z, st))) return rc;
            SpmvArgs q;
            q.x = s->z;
            q.y = s->w;
            q.partials = s->pre->partials;  // z . w, unused
            q.stream_part = s->pre->stream_part;
            q.stop_iter = &s->state.dev()->stop_iter;
            q.it = it;
            if ((rc = launch_spmv(A, kSpmvDot, q, s->variant, st))) return rc;
            double *hcol = s->H + (size_t)j * (size_t)(m + 1);
            for (int i = 0; i <= j + 1; ++i) {
                // pass i: subtract the component along v_{i-1}, start the dot with v_i (or w.w)
                const double *vprev = i > 0 ? s->V + (size_t)(i - 1) * (size_t)s->ldv : nullptr;
                const double *vnext = i <= j ? s->V + (size_t)i * (size_t)s->ldv : nullptr;
                hipLaunchKernelGGL(gmres_project_kernel, dim3(gv), dim3(kBlock), 0, st, n, s->w, vprev, vnext,
                                   bank[(i + 1) & 1], gv, bank[i & 1], i > 0 ? hcol + (i - 1) : nullptr, s->state.dev(), it);
            }
            hipLaunchKernelGGL(gmres_finish_kernel, dim3(gv), dim3(kBlock), 0, st, n, s->w,
                               s->V + (size_t)(j + 1) * (size_t)s->ldv, bank[(j + 1) & 1], gv, s->H, s->cs, s->sn, s->g,
                               m, j, s->state.dev(), it, rtol);
        }
        // ---- x += M^-1 (V y) ----
        hipLaunchKernelGGL(gmres_combine_kernel, dim3(gv), dim3(kBlock), sizeof(double) * (size_t)m, st, n, s->V,
                           s->ldv, s->w, s->H, s->g, m, launched, s->state.dev(), it_base);
        if ((rc = precond_apply(s->pre, s->w, s->z, st))) return rc;
        hipLaunchKernelGGL(gmres_axpy_kernel, dim3(gv), dim3(kBlock), 0, st, n, d_x, s->z, s->state.dev(), it_base);
        SCHWZ_HIP_TRY(hipGetLastError());
        if (it_base + launched >= max_iters) break;
        // the host reads the state one cycle behind the launches
        if ((rc = s->state.poll(st, &stopped))) return rc;
    }
    if (h_iters || h_resnorm) {
        if (const int rc = s->state.read(st)) return rc;
        if (h_iters) *h_iters = s->state.host(0).iters;
        if (h_resnorm) *h_resnorm = s->state.host(0).resn;
    }
    return SCHWZ_OK;
}

}  // extern "C"
