// A new right-hand side on a subdomain that is set up (gfx950, wave64): an extension -- the reference solves the one
// system its initialize() was handed, so no line of it is replaced.  Everything schwz_subdomain_to_device and
// schwz_ras_coarse_set_aggregates build depends on the matrix and the partition alone, except
//   d_rhs                       schwz_ras_rhs_set (host or device values in local order), schwz_ras_rhs_gather (a global
//                               vector in HBM through an index map of 8 B per local row, uploaded at the first gather)
//   beta of the coarse part     schwz_ras_rhs_aggregate: beta_a = sum_{i in a} b_i, one lane per aggregate, the rows of an
//                               aggregate in ascending order into one accumulator -- the order of plan_coarse
//                               (coarse_plan.cpp), so the bits are those of a fresh plan.  The rows grouped by aggregate
//                               (4 B per interior row) are ensure_agg_rows' (coarse.hip), built at the first call.
//   ||b||^2 of the owned rows   schwz_ras_rhs_norm_sq, in block_sum's fixed order
//   d_btilde, x~, y             schwz_ras_restart (subdomain.hip, which knows where y lives) through launch_restart here
// All of them are plain streaming passes on the caller's stream: they run once per solve, not once per step.
#include <hip/hip_runtime.h>

#include "device_utils.hpp"

using namespace schwz;

namespace schwz {

// rhs[i] = global[index[i]]: one indexed load per row
__global__ __launch_bounds__(kBlock) void rhs_gather_kernel(int64_t n, const int64_t *__restrict__ index,
                                                            const double *__restrict__ global, double *__restrict__ rhs)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) rhs[i] = global[index[i]];
}

// one lane per aggregate; additions only (nothing to contract), rows ascending, one accumulator from +0.0
__global__ __launch_bounds__(kBlock) void rhs_aggregate_kernel(int m, const int32_t *__restrict__ agg_ptr,
                                                               const int32_t *__restrict__ agg_rows,
                                                               const double *__restrict__ rhs, double *__restrict__ beta)
{
    const int a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= m) return;
    double t = 0.0;
    for (int q = agg_ptr[a]; q < agg_ptr[a + 1]; ++q) t += rhs[agg_rows[q]];
    beta[a] = t;
}

// partial[block] = sum of b_i^2 over the block's grid-stride share of [0, n), 16-byte loads, the odd last entry with
// workgroup 0
__global__ __launch_bounds__(kBlock) void rhs_norm_sq_kernel(int64_t n, const double *__restrict__ b,
                                                             double *__restrict__ partial)
{
    __shared__ double red[4];
    const int64_t pairs = n >> 1, stride = (int64_t)gridDim.x * kBlock;
    const vd2 *b2 = reinterpret_cast<const vd2 *>(b);
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < pairs; i += stride) {
        const vd2 v = b2[i];
        s += v.x * v.x;
        s += v.y * v.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) s += b[n - 1] * b[n - 1];
    s = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// x[0:nx] = 0, x_alt[0:nx] = 0 and y[0:n] = 0 where they exist, bt[0:n] = b[0:n] (n <= nx): 16-byte stores, the odd
// last entries with workgroup 0
__global__ __launch_bounds__(kBlock) void restart_kernel(int64_t n, int64_t nx, const double *__restrict__ b,
                                                         double *__restrict__ bt, double *__restrict__ x,
                                                         double *__restrict__ x_alt, double *__restrict__ y)
{
    const int64_t pairs_x = nx >> 1, pairs = n >> 1, stride = (int64_t)gridDim.x * kBlock;
    vd2 zero;
    zero.x = zero.y = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < pairs_x; i += stride) {
        store2<false>(x, i, zero);
        if (x_alt) store2<false>(x_alt, i, zero);
        if (i < pairs) {
            store2<false>(bt, i, reinterpret_cast<const vd2 *>(b)[i]);
            if (y) store2<false>(y, i, zero);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (nx & 1) {
            x[nx - 1] = 0.0;
            if (x_alt) x_alt[nx - 1] = 0.0;
        }
        if (n & 1) {
            bt[n - 1] = b[n - 1];
            if (y) y[n - 1] = 0.0;
        }
    }
}

int launch_restart(int64_t n, int64_t nx, const double *b, double *bt, double *x, double *x_alt, double *y, hipStream_t st)
{
    SCHWZ_REQUIRE(n >= 0 && nx >= n && x && (n == 0 || (b && bt)), "launch_restart: bad arguments");
    if (nx == 0) return SCHWZ_OK;
    hipLaunchKernelGGL(restart_kernel, dim3(grid_for((nx + 1) / 2)), dim3(kBlock), 0, st, n, nx, b, bt, x, x_alt, y);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

// the map of schwz_ras_rhs_gather in HBM, uploaded at its first use (the host vector outlives the copy: the stream is
// waited for, once)
static int ensure_rhs_index(schwz_subdomain *sd, hipStream_t st)
{
    if (sd->dev->d_rhs_index) return SCHWZ_OK;
    const size_t n = (size_t)sd->local_size_x;
    const int64_t *h = sd->rhs_index_custom ? sd->rhs_index.data() : sd->l2g.data();
    Dev<int64_t> d;
    int rc;
    if ((rc = d.alloc(n ? n : 1))) return rc;
    if (n) SCHWZ_HIP_TRY(hipMemcpyAsync(d, h, n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    SCHWZ_HIP_TRY(hipStreamSynchronize(st));
    sd->dev->d_rhs_index = std::move(d);
    return SCHWZ_OK;
}

}  // namespace schwz

extern "C" {

int schwz_ras_rhs_set(schwz_subdomain *sd, const double *rhs, int on_device, schwz_stream stream)
{
    SCHWZ_REQUIRE(sd && sd->dev, "schwz_ras_rhs_set: subdomain is not on the device");
    SCHWZ_REQUIRE(rhs, "schwz_ras_rhs_set: null right-hand side");
    const int64_t n = sd->local_size_x;
    if (n == 0) return SCHWZ_OK;
    if (on_device) return launch_copy(n, rhs, sd->dev->d_rhs, (hipStream_t)stream);
    // (waited for: the runtime may read pageable memory after the call returns, and the array is the caller's again)
    SCHWZ_HIP_TRY(hipMemcpyAsync(sd->dev->d_rhs, rhs, (size_t)n * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream));
    SCHWZ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return SCHWZ_OK;
}

int schwz_ras_rhs_index(schwz_subdomain *sd, const int64_t *h_index)
{
    SCHWZ_REQUIRE(sd && sd->dev, "schwz_ras_rhs_index: subdomain is not on the device");
    const size_t n = (size_t)sd->local_size_x;
    if (h_index)
        for (size_t i = 0; i < n; ++i)
            SCHWZ_REQUIRE(h_index[i] >= 0 && h_index[i] < sd->N, "schwz_ras_rhs_index: an index lies outside [0, n_global)");
    // (a gather that still reads the old map on some stream must finish before the map is released)
    if (sd->dev->d_rhs_index) {
        SCHWZ_HIP_TRY(hipDeviceSynchronize());
        sd->dev->d_rhs_index = Dev<int64_t>();
    }
    sd->rhs_index_custom = h_index != nullptr;
    if (h_index)
        sd->rhs_index.assign(h_index, h_index + n);
    else
        std::vector<int64_t>().swap(sd->rhs_index);
    return SCHWZ_OK;
}

int schwz_ras_rhs_gather(schwz_subdomain *sd, const double *d_global, int64_t n_global, schwz_stream stream)
{
    SCHWZ_REQUIRE(sd && sd->dev, "schwz_ras_rhs_gather: subdomain is not on the device");
    SCHWZ_REQUIRE(d_global, "schwz_ras_rhs_gather: null global vector");
    SCHWZ_REQUIRE(n_global == sd->N, "schwz_ras_rhs_gather: the global vector must have one entry per global row");
    const int64_t n = sd->local_size_x;
    if (n == 0) return SCHWZ_OK;
    hipStream_t st = (hipStream_t)stream;
    const int rc = ensure_rhs_index(sd, st);
    if (rc) return rc;
    hipLaunchKernelGGL(rhs_gather_kernel, dim3(grid_for(n)), dim3(kBlock), 0, st, n, (const int64_t *)sd->dev->d_rhs_index, d_global,
                       sd->dev->d_rhs);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_ras_rhs_aggregate(schwz_subdomain *sd, schwz_stream stream)
{
    SCHWZ_REQUIRE(sd && sd->dev, "schwz_ras_rhs_aggregate: subdomain is not on the device");
    schwz_coarse_part *p = sd->dev->coarse;
    if (!p || p->m == 0) return SCHWZ_OK;
    hipStream_t st = (hipStream_t)stream;
    const int rc = ensure_agg_rows(sd, st);
    if (rc) return rc;
    hipLaunchKernelGGL(rhs_aggregate_kernel, dim3((p->m + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (int)p->m,
                       (const int32_t *)p->agg_ptr, (const int32_t *)p->agg_rows, (const double *)sd->dev->d_rhs, (double *)p->beta);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

// sum of b_i^2 over the first n local rows, to the host
static int rhs_norm_sq_rows(schwz_subdomain *sd, int64_t n, double *h_out, schwz_stream stream)
{
    *h_out = 0.0;
    if (n == 0) return SCHWZ_OK;
    hipStream_t st = (hipStream_t)stream;
    const int g = grid_for((n + 1) / 2);
    hipLaunchKernelGGL(rhs_norm_sq_kernel, dim3(g), dim3(kBlock), 0, st, n, (const double *)sd->dev->d_rhs, sd->dev->d_partials);
    SCHWZ_HIP_TRY(hipGetLastError());
    // (slot 1 of the mapped scalars: slot 0 may hold a check norm somebody has not waited for yet)
    const int rc = launch_final_norm(sd->dev->d_partials, g, sd->dev->d_h_scalar + 1, st);
    if (rc) return rc;
    SCHWZ_HIP_TRY(hipStreamSynchronize(st));
    *h_out = sd->dev->h_scalar.p[1];
    return SCHWZ_OK;
}

int schwz_ras_rhs_norm_sq(schwz_subdomain *sd, double *h_out, schwz_stream stream)
{
    SCHWZ_REQUIRE(sd && sd->dev, "schwz_ras_rhs_norm_sq: subdomain is not on the device");
    SCHWZ_REQUIRE(h_out, "schwz_ras_rhs_norm_sq: null output");
    return rhs_norm_sq_rows(sd, sd->local_size, h_out, stream);
}

int schwz_ras_rhs_norm_sq_local(schwz_subdomain *sd, double *h_out, schwz_stream stream)
{
    SCHWZ_REQUIRE(sd && sd->dev, "schwz_ras_rhs_norm_sq_local: subdomain is not on the device");
    SCHWZ_REQUIRE(h_out, "schwz_ras_rhs_norm_sq_local: null output");
    return rhs_norm_sq_rows(sd, sd->local_size_x, h_out, stream);
}

}  // extern "C"
