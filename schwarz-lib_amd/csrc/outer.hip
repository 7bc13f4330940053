// The device half of the outer FGMRES (an extension, include/schwz_hip.h "Outer FGMRES"): the Krylov basis V, the
// preconditioned directions Z, w and a copy of b as vectors over ALL interior rows of the process, and the vector
// passes of one outer iteration -- classical Gram-Schmidt applied twice in three passes whatever j is:
//   A  h  = V^T w, w . w                                      (outer_dots_kernel, outer_fold_kernel)
//   B  w -= V h, then h' = V^T w and w . w in the same launch   (outer_sub_kernel<.., true>, outer_fold_kernel)
//   C  the same launch with h': its dots are the loss of orthogonality, its w . w the square of H(j+1, j)
// The model is the blocked orthogonalisation of the compressed-basis GMRES (gmres.hip, cb_*), with fp64 columns and
// the coefficients handed over by value: the Givens rotations live on the host, which waits for every h anyway.
// Bandwidth kernels: a lane works on two consecutive rows (one 16-byte load per column), all loads of a row pair are
// requested before the first is used, up to kOuterCols accumulators stay in registers so that w and every column are
// read once per pass, grids are capped and grid-stride beyond.  Per-workgroup partial sums, one fp64 value per
// (coefficient, workgroup), are folded by a launch with one workgroup per coefficient in a fixed order: no atomics,
// the same bits on every run.  Bytes of iteration j: 3 * 8 n (j + 2) for the columns and w read, 16 n for w written
// twice, 16 n for the normalisation (w read, V_(j+1) written): 3 * 8 n (j + 2) + 32 n.
//
// A single-basis object (schwz_outer_create_basis, basis 1) keeps V -- and only V -- in fp32: the rounded vector IS the
// basis vector (start and normalize store fl32(w * s), the sweep, the dots and the projections see its widened value),
// all arithmetic stays fp64.  The passes are the *_f32 kernels below, of the same design, a lane on FOUR consecutive
// rows so that a column is still one 16-byte load (w: two): 32 columns in 128 VGPRs beside 64 of accumulators, as the
// fp64 kernels have them.  Bytes of iteration j: three passes over j + 1 columns of 4 n and w of 8 n, w written twice,
// the normalisation reading 8 n and writing 4 n: 3 * (4 n (j + 1) + 8 n) + 16 n + 12 n = 12 n (j + 1) + 52 n, which is
// 0.53 x the fp64 bytes at j = 29 and 0.56 x over a cycle of 30; memory (m + 1) * 4 n + (m + 3) * 8 n against
// (2 m + 4) * 8 n.  Z stays fp64: its rounding error would reach the residual as A (Z^ - Z) y, and it is read once a
// cycle.
#include "device_utils.hpp"

namespace schwz {

constexpr int kOuterCols = 32;        // coefficients of one launch (register blocks of 8)
constexpr int kOuterMaxGrid = 1024;   // four workgroups per CU
constexpr int kOuterMaxRestart = 128;

struct OuterCoef {
    double h[kOuterCols];
};

static int outer_grid(int64_t n)
{
    int64_t g = (n + 2 * (int64_t)kBlock - 1) / (2 * (int64_t)kBlock);
    if (g > kOuterMaxGrid) g = kOuterMaxGrid;
    return g < 1 ? 1 : (int)g;
}

// rows r, r + 1 of a vector (r even, r < n; the vector 16-byte aligned unless !VEC); a row past n reads as zero
template <bool VEC = true>
__device__ __forceinline__ vd2 outer_load(const double *p, int64_t r, int64_t n)
{
    if (VEC && r + 2 <= n) return *reinterpret_cast<const vd2 *>(p + r);
    vd2 v;
    v.x = p[r];
    v.y = r + 1 < n ? p[r + 1] : 0.0;
    return v;
}

template <bool VEC = true>
__device__ __forceinline__ void outer_store(double *p, int64_t r, int64_t n, vd2 v)
{
    if (VEC && r + 2 <= n) {
        *reinterpret_cast<vd2 *>(p + r) = v;
    } else {
        p[r] = v.x;
        if (r + 1 < n) p[r + 1] = v.y;
    }
}

// the workgroup's sums of acc[0 .. 8 NB) to part[k * gridDim.x + blockIdx.x], k < cnt, and of aw to part_ww
template <int NB>
__device__ __forceinline__ void outer_reduce(double (&acc)[8 * NB], double aw, int cnt, double *part, double *part_ww,
                                             double *red)
{
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (8 * b < cnt) {  // (uniform)
            double t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = acc[8 * b + k];
            block_sum_lds<8>(t, red);
            if (threadIdx.x == 0) {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (8 * b + k < cnt) part[(size_t)(8 * b + k) * gridDim.x + blockIdx.x] = t[k];
            }
        }
    }
    if (part_ww) {
        aw = block_sum(aw, red);
        if (threadIdx.x == 0) part_ww[blockIdx.x] = aw;
    }
}

// pass A: this workgroup's share of w . V_k for the cnt <= 8 NB columns at V, and of w . w where part_ww is given
template <int NB>
__global__ __launch_bounds__(kBlock) void outer_dots_kernel(int64_t n, const double *__restrict__ w,
                                                            const double *__restrict__ V, int64_t ld, int cnt,
                                                            double *__restrict__ part, double *__restrict__ part_ww)
{
    __shared__ double red[4 * 8];
    double acc[8 * NB];
#pragma unroll
    for (int k = 0; k < 8 * NB; ++k) acc[k] = 0.0;
    double aw = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; r < n; r += stride) {
        const vd2 wv = outer_load(w, r, n);
        vd2 v[8 * NB];
#pragma unroll
        for (int k = 0; k < 8 * NB; ++k)
            if (k < cnt) v[k] = outer_load(V + (size_t)k * (size_t)ld, r, n);
#pragma unroll
        for (int k = 0; k < 8 * NB; ++k)
            if (k < cnt) acc[k] += wv.x * v[k].x + wv.y * v[k].y;
        aw += wv.x * wv.x + wv.y * wv.y;
    }
    outer_reduce<NB>(acc, aw, cnt, part, part_ww, red);
}

// passes B and C: w -= sum_k h_k V_k over the cnt columns at V, in column order; with DOTS the dots of the new w with
// the same columns, whose values the lane still holds, and its w . w (w is read and written through one pointer)
template <int NB, bool DOTS>
__global__ __launch_bounds__(kBlock) void outer_sub_kernel(int64_t n, double *w, const double *__restrict__ V, int64_t ld,
                                                           int cnt, OuterCoef h, double *__restrict__ part,
                                                           double *__restrict__ part_ww)
{
    __shared__ double red[4 * 8];
    double acc[8 * NB];
#pragma unroll
    for (int k = 0; k < 8 * NB; ++k) acc[k] = 0.0;
    double aw = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; r < n; r += stride) {
        vd2 wv = outer_load(w, r, n);
        vd2 v[8 * NB];
#pragma unroll
        for (int k = 0; k < 8 * NB; ++k)
            if (k < cnt) v[k] = outer_load(V + (size_t)k * (size_t)ld, r, n);
#pragma unroll
        for (int k = 0; k < 8 * NB; ++k) {
            if (k < cnt) {
                wv.x -= h.h[k] * v[k].x;
                wv.y -= h.h[k] * v[k].y;
            }
        }
        outer_store(w, r, n, wv);
        if (DOTS) {
#pragma unroll
            for (int k = 0; k < 8 * NB; ++k)
                if (k < cnt) acc[k] += wv.x * v[k].x + wv.y * v[k].y;
            aw += wv.x * wv.x + wv.y * wv.y;
        }
    }
    if (DOTS) outer_reduce<NB>(acc, aw, cnt, part, part_ww, red);
}

// ---- the passes over fp32 columns -------------------------------------------------------------------------------

typedef float of4 __attribute__((ext_vector_type(4)));

static int outer_grid4(int64_t n)
{
    int64_t g = (n + 4 * (int64_t)kBlock - 1) / (4 * (int64_t)kBlock);
    if (g > kOuterMaxGrid) g = kOuterMaxGrid;
    return g < 1 ? 1 : (int)g;
}

// A trip of a workgroup covers the 4 * kBlock rows from `base` (uniform); a lane takes rows t .. t + 3 of them,
// t = 4 * threadIdx.x, where t < rows = min(n - base, 4 * kBlock).  Addresses are a uniform pointer plus a 32-bit lane
// offset, so a lane keeps no 64-bit address per vector.
//
// rows t .. t + 3 of an fp32 column from `base`: one 16-byte load, no tail form.  The columns belong to the object
// alone: each is padded to a multiple of 64 floats, zeroed at creation, and every store to one (outer_scale_f32_kernel,
// outer_narrow_kernel) stops at row n, so a row past n reads as zero.
__device__ __forceinline__ of4 outer_load4(const float *p, unsigned t)
{
    return *reinterpret_cast<const of4 *>(p + t);
}

// ... of an fp64 vector from `base`, 16-byte aligned: two 16-byte loads; a row past n reads as zero (left = rows - t)
__device__ __forceinline__ void outer_load_w4(const double *p, unsigned t, unsigned left, vd2 &lo, vd2 &hi)
{
    if (left >= 4) {
        lo = *reinterpret_cast<const vd2 *>(p + t);
        hi = *reinterpret_cast<const vd2 *>(p + t + 2);
    } else {
        lo.x = p[t];
        lo.y = left > 1 ? p[t + 1] : 0.0;
        hi.x = left > 2 ? p[t + 2] : 0.0;
        hi.y = 0.0;
    }
}

__device__ __forceinline__ void outer_store_w4(double *p, unsigned t, unsigned left, vd2 lo, vd2 hi)
{
    if (left >= 4) {
        *reinterpret_cast<vd2 *>(p + t) = lo;
        *reinterpret_cast<vd2 *>(p + t + 2) = hi;
    } else {
        p[t] = lo.x;
        if (left > 1) p[t + 1] = lo.y;
        if (left > 2) p[t + 2] = hi.x;
    }
}

// a uniform 64-bit value as scalar registers the loop optimiser cannot fold into per-lane pointers
__device__ __forceinline__ int64_t outer_scalar(int64_t v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ unsigned outer_trip_rows(int64_t n, int64_t base)
{
    const int64_t left = n - base;
    return left < 4 * kBlock ? (unsigned)left : 4u * kBlock;
}

// The widened values of a column live from here to their use only: without it the compiler widens every column of a
// lane at once, or keeps the widened values of the subtraction for the dots -- eight registers per column where the
// loaded floats take four -- and the 32-column forms run out of registers.
__device__ __forceinline__ void outer_pin(of4 &v) { asm volatile("" : "+v"(v)); }

// acc += the four products of a lane's rows, one after the other: one widened value is live at a time
__device__ __forceinline__ void outer_dot4(double &acc, vd2 lo, vd2 hi, of4 v)
{
    acc += lo.x * (double)v.x;
    acc += lo.y * (double)v.y;
    acc += hi.x * (double)v.z;
    acc += hi.y * (double)v.w;
}

// waves per SIMD the fp64 kernels of nb = 1 .. 4 register blocks reach, by kernel: outer_dots_kernel<nb>,
// outer_sub_kernel<nb, true> and outer_sub_kernel<nb, false>.  The fp32 forms are compiled for the same
// (tests/test_outer_basis_resources.py), without scratch.
enum OuterPass { kOuterDots = 0, kOuterSubDots = 1, kOuterSub = 2 };
constexpr int kOuterWaves[3][4] = {{8, 4, 3, 2}, {7, 4, 3, 2}, {8, 6, 4, 3}};
constexpr int outer_waves(OuterPass pass, int nb) { return kOuterWaves[pass][nb - 1]; }

// pass A over fp32 columns: outer_dots_kernel with a lane on four rows
template <int NB>
__global__ __launch_bounds__(kBlock, outer_waves(kOuterDots, NB)) void outer_dots_f32_kernel(
    int64_t n, const double *__restrict__ w, const float *__restrict__ V, int64_t ld, int cnt, double *__restrict__ part,
    double *__restrict__ part_ww)
{
    __shared__ double red[4 * 8];
    double acc[8 * NB];
#pragma unroll
    for (int k = 0; k < 8 * NB; ++k) acc[k] = 0.0;
    double aw = 0.0;
    // (the trip count and each trip's first row are scalars; the lane offset is made opaque once per trip, so that
    // no 64-bit lane address lives across the body: with them this kernel does not fit its twin's registers)
    const int64_t first = (int64_t)blockIdx.x * kBlock * 4, stride = (int64_t)gridDim.x * kBlock * 4;
    const int trips = first < n ? (int)((n - first + stride - 1) / stride) : 0;
#pragma nounroll
    for (int it = 0; it < trips; ++it) {
        const int64_t base = outer_scalar(first + (int64_t)it * stride);
        const unsigned rows = outer_trip_rows(n, base);
        unsigned t = 4u * threadIdx.x;
        asm volatile("" : "+v"(t));
        if (t < rows) {
            const unsigned left = rows - t;
            const double *wp = w + base;
            const float *Vp = V + base;
            // (asked for per trip: hoisted out of the loop, the 8 NB column offsets and the 8 NB masks of k < cnt take
            // more scalar registers than there are, and the overflow is kept in vector registers)
            int64_t ldt = ld;
            int cn = cnt;
            asm volatile("" : "+s"(ldt), "+s"(cn));
            vd2 lo, hi;
            outer_load_w4(wp, t, left, lo, hi);
            of4 v[8 * NB];  // (columns past cnt are zeros: the arithmetic below is straight-line code)
#pragma unroll
            for (int k = 0; k < 8 * NB; ++k) {
                v[k] = of4{0.0f, 0.0f, 0.0f, 0.0f};
                if (k < cn) v[k] = outer_load4(Vp + (size_t)k * (size_t)ldt, t);
            }
#pragma unroll
            for (int k = 0; k < 8 * NB; ++k) {
                outer_pin(v[k]);
                outer_dot4(acc[k], lo, hi, v[k]);
            }
            aw += (lo.x * lo.x + lo.y * lo.y) + (hi.x * hi.x + hi.y * hi.y);
        }
    }
    outer_reduce<NB>(acc, aw, cnt, part, part_ww, red);
}

// passes B and C over fp32 columns: outer_sub_kernel with a lane on four rows, the columns widened exactly
template <int NB, bool DOTS>
__global__ __launch_bounds__(kBlock, outer_waves(DOTS ? kOuterSubDots : kOuterSub, NB)) void outer_sub_f32_kernel(
    int64_t n, double *w, const float *__restrict__ V, int64_t ld, int cnt, OuterCoef h, double *__restrict__ part,
    double *__restrict__ part_ww)
{
    __shared__ double red[4 * 8];
    double acc[8 * NB];
#pragma unroll
    for (int k = 0; k < 8 * NB; ++k) acc[k] = 0.0;
    double aw = 0.0;
    const int64_t first = (int64_t)blockIdx.x * kBlock * 4, stride = (int64_t)gridDim.x * kBlock * 4;
    const int trips = first < n ? (int)((n - first + stride - 1) / stride) : 0;
#pragma nounroll
    for (int it = 0; it < trips; ++it) {
        const int64_t base = outer_scalar(first + (int64_t)it * stride);
        const unsigned rows = outer_trip_rows(n, base);
        unsigned t = 4u * threadIdx.x;
        asm volatile("" : "+v"(t));
        if (t < rows) {
            const unsigned left = rows - t;
            double *wp = w + base;
            const float *Vp = V + base;
            // (asked for per trip: hoisted out of the loop, the 8 NB column offsets and the 8 NB masks of k < cnt take
            // more scalar registers than there are, and the overflow is kept in vector registers)
            int64_t ldt = ld;
            int cn = cnt;
            asm volatile("" : "+s"(ldt), "+s"(cn));
            vd2 lo, hi;
            outer_load_w4(wp, t, left, lo, hi);
            of4 v[8 * NB];  // (columns past cnt are zeros: the arithmetic below is straight-line code)
#pragma unroll
            for (int k = 0; k < 8 * NB; ++k) {
                v[k] = of4{0.0f, 0.0f, 0.0f, 0.0f};
                if (k < cn) v[k] = outer_load4(Vp + (size_t)k * (size_t)ldt, t);
            }
#pragma unroll
            for (int k = 0; k < 8 * NB; ++k) {
                outer_pin(v[k]);
                lo.x -= h.h[k] * (double)v[k].x;
                lo.y -= h.h[k] * (double)v[k].y;
                hi.x -= h.h[k] * (double)v[k].z;
                hi.y -= h.h[k] * (double)v[k].w;
            }
            outer_store_w4(wp, t, left, lo, hi);
            if (DOTS) {
#pragma unroll
                for (int k = 0; k < 8 * NB; ++k) {
                    outer_pin(v[k]);
                    outer_dot4(acc[k], lo, hi, v[k]);
                }
                aw += (lo.x * lo.x + lo.y * lo.y) + (hi.x * hi.x + hi.y * hi.y);
            }
        }
    }
    if (DOTS) outer_reduce<NB>(acc, aw, cnt, part, part_ww, red);
}

// dst = fl32(src * s), round to nearest even: the basis vector of a single-basis object
__global__ __launch_bounds__(kBlock) void outer_scale_f32_kernel(int64_t n, const double *__restrict__ src,
                                                                 float *__restrict__ dst, double s)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock * 4;
    const unsigned t = 4u * threadIdx.x;
#pragma nounroll
    for (int64_t base = (int64_t)blockIdx.x * kBlock * 4; base < n; base += stride) {
        const unsigned rows = outer_trip_rows(n, base);
        if (t >= rows) continue;
        vd2 lo, hi;
        outer_load_w4(src + base, t, rows - t, lo, hi);
        of4 v;
        v.x = (float)(lo.x * s);
        v.y = (float)(lo.y * s);
        v.z = (float)(hi.x * s);
        v.w = (float)(hi.y * s);
        float *d = dst + base;
        if (t + 4 <= rows) {
            *reinterpret_cast<of4 *>(d + t) = v;
        } else {
            d[t] = v.x;
            if (t + 1 < rows) d[t + 1] = v.y;
            if (t + 2 < rows) d[t + 2] = v.z;
        }
    }
}

// rows [0, count) between an fp32 column slice and fp64 memory of any 8-byte alignment, a row per lane: the slices are
// the subdomains' interiors, at arbitrary offsets
__global__ __launch_bounds__(kBlock) void outer_widen_kernel(int64_t count, const float *__restrict__ src,
                                                             double *__restrict__ dst)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) dst[i] = (double)src[i];
}

__global__ __launch_bounds__(kBlock) void outer_narrow_kernel(int64_t count, const double *__restrict__ src,
                                                              float *__restrict__ dst)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) dst[i] = (float)src[i];
}

// w = b - t and this workgroup's share of w . w
template <bool VEC>
__global__ __launch_bounds__(kBlock) void outer_residual_kernel(int64_t n, const double *__restrict__ b,
                                                                const double *__restrict__ t, double *__restrict__ w,
                                                                double *__restrict__ part_ww)
{
    __shared__ double red[4];
    double aw = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; r < n; r += stride) {
        const vd2 bv = outer_load(b, r, n), tv = outer_load<VEC>(t, r, n);
        vd2 wv;
        wv.x = bv.x - tv.x;
        wv.y = bv.y - tv.y;
        outer_store(w, r, n, wv);
        aw += wv.x * wv.x + wv.y * wv.y;
    }
    aw = block_sum(aw, red);
    if (threadIdx.x == 0) part_ww[blockIdx.x] = aw;
}

// one workgroup per coefficient: the fold of its nparts partial sums, in a fixed order, to mapped host memory
__global__ __launch_bounds__(kBlock) void outer_fold_kernel(const double *__restrict__ part, int nparts, double *out)
{
    __shared__ double red[4];
    const double s = fold_partials(part + (size_t)blockIdx.x * (size_t)nparts, nparts, red);
    if (threadIdx.x == 0) {
        out[blockIdx.x] = s;
        __threadfence_system();
    }
}

// x += sum_k y_k Z_k over the cnt columns at Z, in column order
template <int NB, bool VEC>
__global__ __launch_bounds__(kBlock) void outer_combine_kernel(int64_t n, double *x, const double *__restrict__ Z,
                                                               int64_t ld, int cnt, OuterCoef y)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; r < n; r += stride) {
        vd2 xv = outer_load<VEC>(x, r, n);
        vd2 v[8 * NB];
#pragma unroll
        for (int k = 0; k < 8 * NB; ++k)
            if (k < cnt) v[k] = outer_load(Z + (size_t)k * (size_t)ld, r, n);
#pragma unroll
        for (int k = 0; k < 8 * NB; ++k) {
            if (k < cnt) {
                xv.x += y.h[k] * v[k].x;
                xv.y += y.h[k] * v[k].y;
            }
        }
        outer_store<VEC>(x, r, n, xv);
    }
}

__global__ __launch_bounds__(kBlock) void outer_scale_kernel(int64_t n, const double *__restrict__ src,
                                                             double *__restrict__ dst, double s)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; r < n; r += stride) {
        vd2 v = outer_load(src, r, n);
        v.x *= s;
        v.y *= s;
        outer_store(dst, r, n, v);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void outer_copy_kernel(int64_t n, const double *__restrict__ src,
                                                            double *__restrict__ dst)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; r < n; r += stride)
        outer_store<VEC>(dst, r, n, outer_load<VEC>(src, r, n));
}

// dst[0:n] = src[0:n] for pointers of any 8-byte alignment (launch_copy wants 16): the interiors of the subdomains sit
// at arbitrary offsets of the concatenated vectors
int launch_copy_any(int64_t n, const double *src, double *dst, hipStream_t st)
{
    if (n == 0) return SCHWZ_OK;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15u) == 0)
        hipLaunchKernelGGL(outer_copy_kernel<true>, dim3(outer_grid(n)), dim3(kBlock), 0, st, n, src, dst);
    else
        hipLaunchKernelGGL(outer_copy_kernel<false>, dim3(outer_grid(n)), dim3(kBlock), 0, st, n, src, dst);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

}  // namespace schwz

using namespace schwz;

struct schwz_outer {
    int64_t n = 0, ld = 0;
    int m = 0;
    // (every buffer frees itself: schwz_outer_destroy is `delete`)
    Dev<double> V, Z, w, b, part;
    int basis = SCHWZ_OUTER_BASIS_F64;
    Dev<float> Vf;   // the basis of a single-basis object: restart + 1 columns of ldf floats (V is not allocated)
    int64_t ldf = 0;
    Pinned<double> h_coef;     // mapped: the folded coefficients of the last pass, m + 2
    double *d_coef = nullptr;  // its device alias (borrowed)
};

int schwz_outer_create(int64_t n, int restart, schwz_outer **out)
{
    return schwz_outer_create_basis(n, restart, SCHWZ_OUTER_BASIS_F64, out);
}

int schwz_outer_create_basis(int64_t n, int restart, int basis, schwz_outer **out)
{
    SCHWZ_REQUIRE(out, "schwz_outer_create: null output");
    *out = nullptr;
    SCHWZ_REQUIRE(n >= 0, "schwz_outer_create: n must be >= 0");
    SCHWZ_REQUIRE(restart >= 1 && restart <= kOuterMaxRestart, "schwz_outer_create: restart must be in 1..128");
    SCHWZ_REQUIRE(basis == SCHWZ_OUTER_BASIS_F64 || basis == SCHWZ_OUTER_BASIS_F32,
                  "schwz_outer_create_basis: basis must be 0 (double) or 1 (single)");
    std::unique_ptr<schwz_outer> o(new schwz_outer);
    o->n = n;
    o->m = restart;
    o->basis = basis;
    o->ld = (std::max<int64_t>(n, 1) + 31) / 32 * 32;   // columns 256-byte aligned
    o->ldf = (std::max<int64_t>(n, 1) + 63) / 64 * 64;  // (fp32 columns too)
    int rc;
    if ((rc = basis == SCHWZ_OUTER_BASIS_F32 ? o->Vf.alloc((size_t)o->ldf * (size_t)(restart + 1), true)
                                             : o->V.alloc((size_t)o->ld * (size_t)(restart + 1), true)) ||
        (rc = o->Z.alloc((size_t)o->ld * (size_t)restart, true)) ||
        (rc = o->w.alloc((size_t)o->ld, true)) || (rc = o->b.alloc((size_t)o->ld, true)) ||
        (rc = o->part.alloc((size_t)(restart + 2) * kOuterMaxGrid)) || (rc = o->h_coef.alloc((size_t)restart + 2, hipHostMallocMapped)))
        return rc;
    SCHWZ_HIP_TRY(hipHostGetDevicePointer((void **)&o->d_coef, o->h_coef.p, 0));
    *out = o.release();
    return SCHWZ_OK;
}

void schwz_outer_destroy(schwz_outer *o) { delete o; }

int schwz_outer_vector(schwz_outer *o, int which, int j, double **d_ptr)
{
    SCHWZ_REQUIRE(o && d_ptr, "schwz_outer_vector: null argument");
    switch (which) {
    case 0:
        SCHWZ_REQUIRE(j >= 0 && j <= o->m, "schwz_outer_vector: V_j exists for 0 <= j <= restart");
        SCHWZ_REQUIRE(o->basis == SCHWZ_OUTER_BASIS_F64,
                      "schwz_outer_vector: the basis of a single-basis object is fp32: schwz_outer_basis_read / _write");
        *d_ptr = o->V + (size_t)j * (size_t)o->ld;
        break;
    case 1:
        SCHWZ_REQUIRE(j >= 0 && j < o->m, "schwz_outer_vector: Z_j exists for 0 <= j < restart");
        *d_ptr = o->Z + (size_t)j * (size_t)o->ld;
        break;
    case 2:
    case 3:
        SCHWZ_REQUIRE(j == 0, "schwz_outer_vector: w and b take j = 0");
        *d_ptr = which == 2 ? o->w : o->b;
        break;
    default: set_error("schwz_outer_vector: unknown vector id"); return SCHWZ_ERR_INVALID;
    }
    return SCHWZ_OK;
}

// V_j = w * s, rounded to fp32 on a single-basis object
static int outer_scale(schwz_outer *o, int j, double s, hipStream_t st)
{
    if (o->n == 0) return SCHWZ_OK;
    if (o->basis == SCHWZ_OUTER_BASIS_F32)
        hipLaunchKernelGGL(outer_scale_f32_kernel, dim3(outer_grid4(o->n)), dim3(kBlock), 0, st, o->n, (const double *)o->w,
                           o->Vf + (size_t)j * (size_t)o->ldf, s);
    else
        hipLaunchKernelGGL(outer_scale_kernel, dim3(outer_grid(o->n)), dim3(kBlock), 0, st, o->n, (const double *)o->w,
                           o->V + (size_t)j * (size_t)o->ld, s);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_outer_start(schwz_outer *o, double inv_beta, schwz_stream stream)
{
    SCHWZ_REQUIRE(o, "schwz_outer_start: null object");
    return outer_scale(o, 0, inv_beta, (hipStream_t)stream);
}

int schwz_outer_normalize(schwz_outer *o, int j, double inv_norm, schwz_stream stream)
{
    SCHWZ_REQUIRE(o, "schwz_outer_normalize: null object");
    SCHWZ_REQUIRE(j >= 0 && j < o->m, "schwz_outer_normalize: j must be in 0..restart-1");
    return outer_scale(o, j + 1, inv_norm, (hipStream_t)stream);
}

namespace {

// the launches of one pass over columns [c0, c0 + cnt) of V, cnt <= kOuterCols, by the number of register blocks
int pass_grid(const schwz_outer *o) { return o->basis == SCHWZ_OUTER_BASIS_F32 ? outer_grid4(o->n) : outer_grid(o->n); }

int launch_dots(schwz_outer *o, int c0, int cnt, bool ww, int nv, int grid, hipStream_t st)
{
    // (only the buffer of the object's basis exists: its columns' address is formed in that branch alone)
    const bool f32 = o->basis == SCHWZ_OUTER_BASIS_F32;
    const double *V = f32 ? nullptr : o->V + (size_t)c0 * (size_t)o->ld;
    const float *Vf = f32 ? o->Vf + (size_t)c0 * (size_t)o->ldf : nullptr;
    double *part = o->part + (size_t)c0 * grid, *pw = ww ? o->part + (size_t)nv * grid : nullptr;
#define SCHWZ_OUTER_DOTS(NB)                                                                                           \
    do {                                                                                                               \
        if (f32)                                                                                                       \
            hipLaunchKernelGGL(outer_dots_f32_kernel<NB>, dim3(grid), dim3(kBlock), 0, st, o->n, (const double *)o->w, Vf, o->ldf, cnt, part, pw); \
        else                                                                                                           \
            hipLaunchKernelGGL(outer_dots_kernel<NB>, dim3(grid), dim3(kBlock), 0, st, o->n, (const double *)o->w, V, o->ld, cnt, part, pw); \
    } while (0)
    switch ((cnt + 7) / 8) {
    case 1: SCHWZ_OUTER_DOTS(1); break;
    case 2: SCHWZ_OUTER_DOTS(2); break;
    case 3: SCHWZ_OUTER_DOTS(3); break;
    default: SCHWZ_OUTER_DOTS(4); break;
    }
#undef SCHWZ_OUTER_DOTS
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

template <bool DOTS>
int launch_sub(schwz_outer *o, int c0, int cnt, const double *h, int nv, int grid, hipStream_t st)
{
    const bool f32 = o->basis == SCHWZ_OUTER_BASIS_F32;
    const double *V = f32 ? nullptr : o->V + (size_t)c0 * (size_t)o->ld;
    const float *Vf = f32 ? o->Vf + (size_t)c0 * (size_t)o->ldf : nullptr;
    double *part = o->part + (size_t)c0 * grid, *pw = o->part + (size_t)nv * grid;
    OuterCoef c;
    for (int k = 0; k < kOuterCols; ++k) c.h[k] = k < cnt ? h[c0 + k] : 0.0;
#define SCHWZ_OUTER_SUB(NB)                                                                                            \
    do {                                                                                                               \
        if (f32)                                                                                                       \
            hipLaunchKernelGGL((outer_sub_f32_kernel<NB, DOTS>), dim3(grid), dim3(kBlock), 0, st, o->n, (double *)o->w, Vf, o->ldf, cnt, c, part, pw); \
        else                                                                                                           \
            hipLaunchKernelGGL((outer_sub_kernel<NB, DOTS>), dim3(grid), dim3(kBlock), 0, st, o->n, (double *)o->w, V, o->ld, cnt, c, part, pw); \
    } while (0)
    switch ((cnt + 7) / 8) {
    case 1: SCHWZ_OUTER_SUB(1); break;
    case 2: SCHWZ_OUTER_SUB(2); break;
    case 3: SCHWZ_OUTER_SUB(3); break;
    default: SCHWZ_OUTER_SUB(4); break;
    }
#undef SCHWZ_OUTER_SUB
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

// the nv + 1 folded coefficients of the pass that has just been launched, to the host
int fold_to_host(schwz_outer *o, int nv, int grid, double *h_out, hipStream_t st)
{
    hipLaunchKernelGGL(outer_fold_kernel, dim3(nv + 1), dim3(kBlock), 0, st, (const double *)o->part, grid, o->d_coef);
    SCHWZ_HIP_TRY(hipGetLastError());
    SCHWZ_HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(h_out, o->h_coef.p, (size_t)(nv + 1) * sizeof(double));
    return SCHWZ_OK;
}

}  // namespace

int schwz_outer_dots(schwz_outer *o, int j, double *h_out, schwz_stream stream)
{
    SCHWZ_REQUIRE(o && h_out, "schwz_outer_dots: null argument");
    SCHWZ_REQUIRE(j >= 0 && j < o->m, "schwz_outer_dots: j must be in 0..restart-1");
    hipStream_t st = (hipStream_t)stream;
    const int nv = j + 1;
    if (o->n == 0) {
        std::memset(h_out, 0, (size_t)(nv + 1) * sizeof(double));
        return SCHWZ_OK;
    }
    const int grid = pass_grid(o);
    int rc;
    for (int c0 = 0; c0 < nv; c0 += kOuterCols)
        if ((rc = launch_dots(o, c0, std::min(kOuterCols, nv - c0), c0 == 0, nv, grid, st))) return rc;
    return fold_to_host(o, nv, grid, h_out, st);
}

int schwz_outer_project_dots(schwz_outer *o, int j, const double *h_in, double *h_out, schwz_stream stream)
{
    SCHWZ_REQUIRE(o && h_in && h_out, "schwz_outer_project_dots: null argument");
    SCHWZ_REQUIRE(j >= 0 && j < o->m, "schwz_outer_project_dots: j must be in 0..restart-1");
    hipStream_t st = (hipStream_t)stream;
    const int nv = j + 1;
    if (o->n == 0) {
        std::memset(h_out, 0, (size_t)(nv + 1) * sizeof(double));
        return SCHWZ_OK;
    }
    const int grid = pass_grid(o);
    int rc;
    if (nv <= kOuterCols) {
        if ((rc = launch_sub<true>(o, 0, nv, h_in, nv, grid, st))) return rc;
    } else {
        // more columns than one launch holds: the subtraction is complete before the first dot is taken
        for (int c0 = 0; c0 < nv; c0 += kOuterCols)
            if ((rc = launch_sub<false>(o, c0, std::min(kOuterCols, nv - c0), h_in, nv, grid, st))) return rc;
        for (int c0 = 0; c0 < nv; c0 += kOuterCols)
            if ((rc = launch_dots(o, c0, std::min(kOuterCols, nv - c0), c0 == 0, nv, grid, st))) return rc;
    }
    return fold_to_host(o, nv, grid, h_out, st);
}

int schwz_outer_combine(schwz_outer *o, int k, const double *h_y, double *d_x, schwz_stream stream)
{
    SCHWZ_REQUIRE(o && h_y, "schwz_outer_combine: null argument");
    SCHWZ_REQUIRE(k >= 1 && k <= o->m, "schwz_outer_combine: k must be in 1..restart");
    SCHWZ_REQUIRE(d_x || o->n == 0, "schwz_outer_combine: null x");
    if (o->n == 0) return SCHWZ_OK;
    hipStream_t st = (hipStream_t)stream;
    const int grid = outer_grid(o->n);
    const bool vec = ((uintptr_t)d_x & 15u) == 0;
    for (int c0 = 0; c0 < k; c0 += kOuterCols) {
        const int cnt = std::min(kOuterCols, k - c0);
        const double *Z = o->Z + (size_t)c0 * (size_t)o->ld;
        OuterCoef c;
        for (int i = 0; i < kOuterCols; ++i) c.h[i] = i < cnt ? h_y[c0 + i] : 0.0;
#define SCHWZ_OUTER_COMBINE(NB)                                                                                        \
    do {                                                                                                               \
        if (vec)                                                                                                       \
            hipLaunchKernelGGL((outer_combine_kernel<NB, true>), dim3(grid), dim3(kBlock), 0, st, o->n, d_x, Z, o->ld, cnt, c); \
        else                                                                                                           \
            hipLaunchKernelGGL((outer_combine_kernel<NB, false>), dim3(grid), dim3(kBlock), 0, st, o->n, d_x, Z, o->ld, cnt, c); \
    } while (0)
        switch ((cnt + 7) / 8) {
        case 1: SCHWZ_OUTER_COMBINE(1); break;
        case 2: SCHWZ_OUTER_COMBINE(2); break;
        case 3: SCHWZ_OUTER_COMBINE(3); break;
        default: SCHWZ_OUTER_COMBINE(4); break;
        }
#undef SCHWZ_OUTER_COMBINE
        SCHWZ_HIP_TRY(hipGetLastError());
    }
    return SCHWZ_OK;
}

int schwz_outer_copy(int64_t n, const double *d_src, double *d_dst, schwz_stream stream)
{
    SCHWZ_REQUIRE(n >= 0, "schwz_outer_copy: n must be >= 0");
    SCHWZ_REQUIRE((d_src && d_dst) || n == 0, "schwz_outer_copy: null argument");
    return launch_copy_any(n, d_src, d_dst, (hipStream_t)stream);
}

int schwz_outer_residual(schwz_outer *o, const double *d_t, double *h_out, schwz_stream stream)
{
    SCHWZ_REQUIRE(o && h_out, "schwz_outer_residual: null argument");
    SCHWZ_REQUIRE(d_t || o->n == 0, "schwz_outer_residual: null t");
    if (o->n == 0) {
        h_out[0] = 0.0;
        return SCHWZ_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    const int grid = outer_grid(o->n);
    if (((uintptr_t)d_t & 15u) == 0)
        hipLaunchKernelGGL(outer_residual_kernel<true>, dim3(grid), dim3(kBlock), 0, st, o->n, (const double *)o->b, d_t,
                           (double *)o->w, (double *)o->part);
    else
        hipLaunchKernelGGL(outer_residual_kernel<false>, dim3(grid), dim3(kBlock), 0, st, o->n, (const double *)o->b, d_t,
                           (double *)o->w, (double *)o->part);
    SCHWZ_HIP_TRY(hipGetLastError());
    return fold_to_host(o, 0, grid, h_out, st);
}

// rows [first, first + count) of V_j checked against the object
static int outer_basis_slice(const schwz_outer *o, int j, int64_t first, int64_t count, const void *d_mem)
{
    SCHWZ_REQUIRE(o, "schwz_outer_basis_read / _write: null object");
    SCHWZ_REQUIRE(j >= 0 && j <= o->m, "schwz_outer_basis_read / _write: V_j exists for 0 <= j <= restart");
    SCHWZ_REQUIRE(first >= 0 && count >= 0 && first <= o->n && count <= o->n - first,
                  "schwz_outer_basis_read / _write: rows first .. first + count must lie in 0 .. n");
    SCHWZ_REQUIRE(d_mem || count == 0, "schwz_outer_basis_read / _write: null device pointer");
    return SCHWZ_OK;
}

static int outer_slice_grid(int64_t count)
{
    const int64_t g = (count + kBlock - 1) / kBlock;
    return (int)std::min<int64_t>(g, 4 * kOuterMaxGrid);
}

int schwz_outer_basis_read(schwz_outer *o, int j, int64_t first, int64_t count, double *d_dst, schwz_stream stream)
{
    int rc;
    if ((rc = outer_basis_slice(o, j, first, count, d_dst))) return rc;
    if (count == 0) return SCHWZ_OK;
    if (o->basis == SCHWZ_OUTER_BASIS_F64)
        return launch_copy_any(count, o->V + (size_t)j * (size_t)o->ld + first, d_dst, (hipStream_t)stream);
    hipLaunchKernelGGL(outer_widen_kernel, dim3(outer_slice_grid(count)), dim3(kBlock), 0, (hipStream_t)stream, count,
                       (const float *)(o->Vf + (size_t)j * (size_t)o->ldf + first), d_dst);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_outer_basis_write(schwz_outer *o, int j, int64_t first, int64_t count, const double *d_src, schwz_stream stream)
{
    int rc;
    if ((rc = outer_basis_slice(o, j, first, count, d_src))) return rc;
    if (count == 0) return SCHWZ_OK;
    if (o->basis == SCHWZ_OUTER_BASIS_F64)
        return launch_copy_any(count, d_src, o->V + (size_t)j * (size_t)o->ld + first, (hipStream_t)stream);
    hipLaunchKernelGGL(outer_narrow_kernel, dim3(outer_slice_grid(count)), dim3(kBlock), 0, (hipStream_t)stream, count,
                       d_src, o->Vf + (size_t)j * (size_t)o->ldf + first);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}
