// Aggregation coarse correction of the two-level RAS iteration (gfx950, wave64), ahead of the unchanged RAS step:
//     x <- x + Z A0^-1 Z^T (b - A x),   A0 = Z^T A Z
// as three kinds of launches per outer step (the plan of every table is coarse_plan.cpp's):
//   residual  s[first_agg + a] = beta_a - sum_j W_aj x~[slot_j]   per subdomain: one workgroup per piece of at most
//             kCoarsePieceCap entries reduces in block_sum's fixed tree order and stores one partial sum; a second
//             small launch folds the pieces of every aggregate in table order.  No atomics: the same bits from run
//             to run, whatever the grid.
//   solve     c = A0^-1 s, a dense fp64 GEMV over the explicit inverse, once per process: one wave per row,
//             16-byte loads, the wave's 64 partial sums folded by wave_sum.  Bound by the nc^2 * 8 bytes of the inverse.
//   apply     x~[j] += c[id16[j]] over every slot and y[j] += c[id16[j]] over local_size_x in ONE pass, c staged in
//             LDS (at most 32 KiB); where y is the x~ buffer itself the pass adds once (schwz_ras_coarse_apply,
//             subdomain.hip, knows where y lives).
#include <hip/hip_runtime.h>

#include "coarse_plan.hpp"
#include "device_utils.hpp"

using namespace schwz;

namespace schwz {

__global__ __launch_bounds__(kBlock) void coarse_partial_kernel(const int32_t *__restrict__ piece,
                                                                const int32_t *__restrict__ w_slot,
                                                                const double *__restrict__ w_val,
                                                                const double *__restrict__ x, double *__restrict__ partial)
{
    __shared__ double red[4];
    const int p = blockIdx.x;
    const int begin = piece[3 * p + 1], end = piece[3 * p + 2];
    double s = 0.0;
    for (int k = begin + (int)threadIdx.x; k < end; k += kBlock) s += w_val[k] * x[w_slot[k]];
    s = block_sum(s, red);
    if (threadIdx.x == 0) partial[p] = s;
}

__global__ __launch_bounds__(kBlock) void coarse_fold_kernel(int m, const double *__restrict__ beta,
                                                             const int32_t *__restrict__ piece_ptr,
                                                             const double *__restrict__ partial, double *__restrict__ s_out)
{
    const int a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= m) return;
    double t = 0.0;
    for (int p = piece_ptr[a]; p < piece_ptr[a + 1]; ++p) t += partial[p];  // table order
    s_out[a] = beta[a] - t;
}

// one wave per row, rows in fixed order; PAIRS: nc is even and the row is read as 16-byte pairs
template <bool PAIRS>
__global__ __launch_bounds__(kBlock) void coarse_gemv_kernel(int nc, const double *__restrict__ inv,
                                                             const double *__restrict__ s, double *__restrict__ c)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= nc) return;  // (whole waves leave: no barrier follows)
    const double *r = inv + (size_t)row * (size_t)nc;
    double acc = 0.0;
    if (PAIRS) {
        const vd2 *r2 = reinterpret_cast<const vd2 *>(r), *s2 = reinterpret_cast<const vd2 *>(s);
        const int half = nc >> 1;
#pragma unroll 4
        for (int k = lane; k < half; k += 64) {
            const vd2 a = __builtin_nontemporal_load(r2 + k), b = s2[k];
            acc += a.x * b.x;
            acc += a.y * b.y;
        }
    } else {
#pragma unroll 4
        for (int k = lane; k < nc; k += 64) acc += r[k] * s[k];
    }
    acc = wave_sum(acc);
    if (lane == 0) c[row] = acc;
}

__global__ __launch_bounds__(kBlock) void coarse_apply_kernel(int nc, const double *__restrict__ c,
                                                              const uint16_t *__restrict__ id16, double *__restrict__ x,
                                                              int64_t nx, double *__restrict__ y, int64_t ny)
{
    extern __shared__ double c_lds[];
    for (int k = threadIdx.x; k < nc; k += kBlock) c_lds[k] = c[k];
    __syncthreads();
    const int64_t pairs = nx >> 1, stride = (int64_t)gridDim.x * kBlock;
    const uint32_t *id2 = reinterpret_cast<const uint32_t *>(id16);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < pairs; i += stride) {
        const uint32_t ids = id2[i];
        vd2 v;
        v.x = c_lds[ids & 0xffffu];
        v.y = c_lds[ids >> 16];
        vd2 *x2 = reinterpret_cast<vd2 *>(x) + i;
        vd2 t = *x2;
        t.x += v.x;
        t.y += v.y;
        *x2 = t;
        if (y) {
            if (2 * i + 1 < ny) {
                vd2 *y2 = reinterpret_cast<vd2 *>(y) + i;
                vd2 u = *y2;
                u.x += v.x;
                u.y += v.y;
                *y2 = u;
            } else if (2 * i < ny) {
                y[2 * i] += v.x;
            }
        }
    }
    if ((nx & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double v = c_lds[id16[nx - 1]];
        x[nx - 1] += v;
        if (y && nx - 1 < ny) y[nx - 1] += v;
    }
}

int launch_coarse_apply(const schwz_coarse_part *part, const schwz_coarse *c, double *x, int64_t nx, double *y, int64_t ny,
                        hipStream_t st)
{
    SCHWZ_REQUIRE(part && c && x && nx == part->nslots && ny <= nx && c->nc == part->nc, "launch_coarse_apply: bad arguments");
    if (nx == 0) return SCHWZ_OK;
    // at least four pairs per lane on large subdomains: every workgroup stages c once
    const int64_t want = ((nx >> 1) + 4 * kBlock - 1) / (4 * kBlock);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, kMaxGrid / 2));
    hipLaunchKernelGGL(coarse_apply_kernel, dim3(grid), dim3(kBlock), (size_t)c->nc * sizeof(double), st, (int)c->nc,
                       (const double *)c->c, (const uint16_t *)part->id16, x, nx, y, ny);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

}  // namespace schwz

extern "C" {

int schwz_coarse_create(int32_t nc, const double *h_inv, schwz_coarse **out)
{
    SCHWZ_REQUIRE(out, "schwz_coarse_create: null output");
    *out = nullptr;
    SCHWZ_REQUIRE(nc >= 1 && nc <= kCoarseMaxDofs,
                  "schwz_coarse_create: the number of aggregates must be in [1, " + std::to_string(kCoarseMaxDofs) + "]");
    SCHWZ_REQUIRE(h_inv, "schwz_coarse_create: null inverse");
    if (schwz_device_count() < 1) {
        set_error("schwz_coarse_create: no HIP device visible (there is no CPU fallback)");
        return SCHWZ_ERR_HIP;
    }
    std::unique_ptr<schwz_coarse> c(new schwz_coarse());
    c->nc = nc;
    int rc;
    // (one spare double behind s and c: the 16-byte loads of an even nc never reach it, an allocation is never empty)
    if ((rc = c->inv.alloc((size_t)nc * (size_t)nc)) || (rc = c->s.alloc((size_t)nc + 1, true)) ||
        (rc = c->c.alloc((size_t)nc + 1, true)))
        return rc;
    SCHWZ_HIP_TRY(hipMemcpy(c->inv, h_inv, (size_t)nc * (size_t)nc * sizeof(double), hipMemcpyHostToDevice));
    *out = c.release();
    return SCHWZ_OK;
}

void schwz_coarse_destroy(schwz_coarse *c) { delete c; }

int schwz_coarse_vector(schwz_coarse *c, int which, double **d_ptr, int32_t *len)
{
    SCHWZ_REQUIRE(c && d_ptr && len, "schwz_coarse_vector: null argument");
    SCHWZ_REQUIRE(which == 0 || which == 1, "schwz_coarse_vector: unknown vector id");
    *d_ptr = which == 0 ? (double *)c->s : (double *)c->c;
    *len = c->nc;
    return SCHWZ_OK;
}

int schwz_coarse_solve(schwz_coarse *c, schwz_stream stream)
{
    SCHWZ_REQUIRE(c, "schwz_coarse_solve: null argument");
    const int nc = c->nc, grid = (nc + kBlock / 64 - 1) / (kBlock / 64);
    if (nc % 2 == 0)
        hipLaunchKernelGGL(coarse_gemv_kernel<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, nc,
                           (const double *)c->inv, (const double *)c->s, (double *)c->c);
    else
        hipLaunchKernelGGL(coarse_gemv_kernel<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, nc,
                           (const double *)c->inv, (const double *)c->s, (double *)c->c);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_ras_coarse_set_aggregates(schwz_subdomain *sd, const int32_t *h_slot_agg, int32_t first_agg, int32_t m, int32_t nc)
{
    SCHWZ_REQUIRE(sd && sd->dev, "schwz_ras_coarse_set_aggregates: subdomain is not on the device");
    if (sd->P > 1 && sd->overlap < 2) {
        // the local matrix of such a subdomain drops the couplings of its interior rows to other subdomains
        set_error("schwz_ras_coarse_set_aggregates: the coarse correction needs overlap >= 2 on more than one subdomain");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    StageTimer timer("coarse plan + upload");
    const int64_t n = sd->local_size, nslots = sd->local_size_x + sd->halo_size;
    std::vector<double> rhs((size_t)n);
    if (n) SCHWZ_HIP_TRY(hipMemcpy(rhs.data(), sd->dev->d_rhs, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    CoarsePlan plan;
    int rc = plan_coarse(n, nslots, sd->l_rp.data(), sd->l_col.data(), sd->l_val.data(), rhs.data(), h_slot_agg, first_agg, m,
                         nc, &plan);
    if (rc) return rc;
    std::unique_ptr<schwz_coarse_part> part(new schwz_coarse_part());
    part->first_agg = first_agg;
    part->m = m;
    part->nc = nc;
    part->nslots = nslots;
    part->nw = (int64_t)plan.w_slot.size();
    part->npieces = (int)plan.pieces.size();
    std::vector<int32_t> piece;
    piece.reserve(plan.pieces.size() * 3);
    for (const CoarsePiece &q : plan.pieces) piece.insert(piece.end(), {q.agg, q.begin, q.end});
    // (id16 is read two ids at a time: one spare id behind an odd count)
    if ((rc = part->beta.put(plan.beta)) || (rc = part->w_val.put(plan.w_val)) || (rc = part->w_slot.put(plan.w_slot)) ||
        (rc = part->piece.put(piece)) || (rc = part->piece_ptr.put(plan.piece_ptr)) || (rc = part->id16.put(plan.id16, 1)) ||
        (rc = part->partial.alloc(plan.pieces.size() + 1, true)))
        return rc;
    part->rows = std::move(plan.rows);
    SCHWZ_HIP_TRY(hipDeviceSynchronize());
    delete sd->dev->coarse;
    sd->dev->coarse = part.release();
    return SCHWZ_OK;
}

int schwz_ras_coarse_rows(const schwz_subdomain *sd, double *h_rows)
{
    SCHWZ_REQUIRE(sd && sd->dev && sd->dev->coarse, "schwz_ras_coarse_rows: the subdomain has no aggregates (schwz_ras_coarse_set_aggregates)");
    SCHWZ_REQUIRE(h_rows || sd->dev->coarse->rows.empty(), "schwz_ras_coarse_rows: null output");
    std::copy(sd->dev->coarse->rows.begin(), sd->dev->coarse->rows.end(), h_rows);
    return SCHWZ_OK;
}

int schwz_ras_coarse_residual(schwz_subdomain *sd, schwz_coarse *c, schwz_stream stream)
{
    SCHWZ_REQUIRE(sd && sd->dev && sd->dev->coarse,
                  "schwz_ras_coarse_residual: the subdomain has no aggregates (schwz_ras_coarse_set_aggregates)");
    const schwz_coarse_part *p = sd->dev->coarse;
    SCHWZ_REQUIRE(c && c->nc == p->nc, "schwz_ras_coarse_residual: the coarse object has another number of aggregates");
    if (p->m == 0) return SCHWZ_OK;
    hipStream_t st = (hipStream_t)stream;
    if (p->npieces > 0) {
        hipLaunchKernelGGL(coarse_partial_kernel, dim3(p->npieces), dim3(kBlock), 0, st, (const int32_t *)p->piece,
                           (const int32_t *)p->w_slot, (const double *)p->w_val, (const double *)sd->dev->d_x,
                           (double *)p->partial);
        SCHWZ_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(coarse_fold_kernel, dim3((p->m + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (int)p->m,
                       (const double *)p->beta, (const int32_t *)p->piece_ptr, (const double *)p->partial,
                       (double *)c->s + p->first_agg);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

}  // extern "C"
