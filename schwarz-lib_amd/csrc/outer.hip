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
    Pinned<double> h_coef;     // mapped: the folded coefficients of the last pass, m + 2
    double *d_coef = nullptr;  // its device alias (borrowed)
};

int schwz_outer_create(int64_t n, int restart, schwz_outer **out)
{
    SCHWZ_REQUIRE(out, "schwz_outer_create: null output");
    *out = nullptr;
    SCHWZ_REQUIRE(n >= 0, "schwz_outer_create: n must be >= 0");
    SCHWZ_REQUIRE(restart >= 1 && restart <= kOuterMaxRestart, "schwz_outer_create: restart must be in 1..128");
    std::unique_ptr<schwz_outer> o(new schwz_outer);
    o->n = n;
    o->m = restart;
    o->ld = (std::max<int64_t>(n, 1) + 31) / 32 * 32;  // columns 256-byte aligned
    int rc;
    if ((rc = o->V.alloc((size_t)o->ld * (size_t)(restart + 1), true)) || (rc = o->Z.alloc((size_t)o->ld * (size_t)restart, true)) ||
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

static int outer_scale(schwz_outer *o, double *dst, double s, hipStream_t st)
{
    if (o->n == 0) return SCHWZ_OK;
    hipLaunchKernelGGL(outer_scale_kernel, dim3(outer_grid(o->n)), dim3(kBlock), 0, st, o->n, (const double *)o->w, dst, s);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_outer_start(schwz_outer *o, double inv_beta, schwz_stream stream)
{
    SCHWZ_REQUIRE(o, "schwz_outer_start: null object");
    return outer_scale(o, o->V, inv_beta, (hipStream_t)stream);
}

int schwz_outer_normalize(schwz_outer *o, int j, double inv_norm, schwz_stream stream)
{
    SCHWZ_REQUIRE(o, "schwz_outer_normalize: null object");
    SCHWZ_REQUIRE(j >= 0 && j < o->m, "schwz_outer_normalize: j must be in 0..restart-1");
    return outer_scale(o, o->V + (size_t)(j + 1) * (size_t)o->ld, inv_norm, (hipStream_t)stream);
}

namespace {

// the launches of one pass over columns [c0, c0 + cnt) of V, cnt <= kOuterCols, by the number of register blocks
int launch_dots(schwz_outer *o, int c0, int cnt, bool ww, int nv, int grid, hipStream_t st)
{
    const double *V = o->V + (size_t)c0 * (size_t)o->ld;
    double *part = o->part + (size_t)c0 * grid, *pw = ww ? o->part + (size_t)nv * grid : nullptr;
#define SCHWZ_OUTER_DOTS(NB) \
    hipLaunchKernelGGL(outer_dots_kernel<NB>, dim3(grid), dim3(kBlock), 0, st, o->n, (const double *)o->w, V, o->ld, cnt, part, pw)
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
    const double *V = o->V + (size_t)c0 * (size_t)o->ld;
    double *part = o->part + (size_t)c0 * grid, *pw = o->part + (size_t)nv * grid;
    OuterCoef c;
    for (int k = 0; k < kOuterCols; ++k) c.h[k] = k < cnt ? h[c0 + k] : 0.0;
#define SCHWZ_OUTER_SUB(NB) \
    hipLaunchKernelGGL((outer_sub_kernel<NB, DOTS>), dim3(grid), dim3(kBlock), 0, st, o->n, (double *)o->w, V, o->ld, cnt, c, part, pw)
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
    const int grid = outer_grid(o->n);
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
    const int grid = outer_grid(o->n);
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
