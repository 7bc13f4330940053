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
// and, for a preconditioner whose right-hand side changes with every application (the outer FGMRES, outer.py),
//   restriction  s[first_agg + a] = sum_{i in a} v[i] for any vector v in local order (schwz_ras_aggregate_sums): the
//             two launches of the residual over the rows grouped by aggregate instead of W -- one workgroup per piece
//             of at most kCoarsePieceCap rows, 8 B of v and 4 B of row id per interior row, then the fold in table
//             order.  beta is neither read nor written.
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

// partial[p] = sum of v over the rows of piece p.  A piece holds at most 8 rows per lane: the row ids, then the values,
// are all asked for before the first addition; a lane adds its rows in ascending order from +0.0 (a row beyond the
// piece adds +0.0, which changes no bit of a sum that started from +0.0)
static_assert(kCoarsePieceCap == 8 * kBlock, "agg_partial_kernel: a lane holds 8 rows of a piece");
__global__ __launch_bounds__(kBlock) void agg_partial_kernel(const int32_t *__restrict__ piece,
                                                             const int32_t *__restrict__ agg_rows,
                                                             const double *__restrict__ v, double *__restrict__ partial)
{
    __shared__ double red[4];
    const int p = blockIdx.x;
    const int begin = piece[3 * p + 1], end = piece[3 * p + 2];
    int32_t row[8];
    double val[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int k = begin + u * kBlock + (int)threadIdx.x;
        row[u] = k < end ? __builtin_nontemporal_load(agg_rows + k) : -1;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) val[u] = row[u] >= 0 ? v[row[u]] : 0.0;
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += val[u];
    s = block_sum(s, red);
    if (threadIdx.x == 0) partial[p] = s;
}

__global__ __launch_bounds__(kBlock) void agg_fold_kernel(int m, const int32_t *__restrict__ piece_ptr,
                                                          const double *__restrict__ partial, double *__restrict__ s_out)
{
    const int a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= m) return;
    double t = 0.0;
    for (int p = piece_ptr[a]; p < piece_ptr[a + 1]; ++p) t += partial[p];  // table order
    s_out[a] = t;
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

int ensure_agg_rows(schwz_subdomain *sd, hipStream_t st)
{
    schwz_coarse_part *p = sd->dev->coarse;
    if (p->agg_ready) return SCHWZ_OK;
    const int64_t n = sd->local_size;
    std::vector<uint16_t> id((size_t)n);
    if (n) {
        SCHWZ_HIP_TRY(hipMemcpyAsync(id.data(), (const uint16_t *)p->id16, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        SCHWZ_HIP_TRY(hipStreamSynchronize(st));
    }
    AggRows g;
    int rc;
    if ((rc = group_rows_by_aggregate(n, id.data(), p->first_agg, p->m, &g)) ||
        (rc = plan_row_pieces(p->m, g.ptr.data(), &g.pieces, &g.piece_ptr)))
        return rc;
    std::vector<int32_t> piece;
    piece.reserve(g.pieces.size() * 3);
    for (const CoarsePiece &q : g.pieces) piece.insert(piece.end(), {q.agg, q.begin, q.end});
    // (put returns when its copy has landed: a launch on any stream may follow; every partial is stored before it is read)
    if ((rc = p->agg_rows.put(g.rows)) || (rc = p->agg_ptr.put(g.ptr)) || (rc = p->row_piece.put(piece)) ||
        (rc = p->row_piece_ptr.put(g.piece_ptr)) || (rc = p->row_partial.alloc(g.pieces.size() + 1)))
        return rc;
    SCHWZ_REQUIRE(p->nrow_pieces == (int32_t)g.pieces.size(), "ensure_agg_rows: the piece table has another length than planned");
    p->agg_ready = true;
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
    {
        // (the count of the row pieces follows from the aggregates' sizes: the byte model knows it before the tables exist)
        std::vector<int32_t> count((size_t)m, 0);
        for (int64_t i = 0; i < n; ++i) ++count[(size_t)(h_slot_agg[i] - first_agg)];
        for (int32_t a = 0; a < m; ++a) part->nrow_pieces += (count[(size_t)a] + kCoarsePieceCap - 1) / kCoarsePieceCap;
    }
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

int schwz_ras_aggregate_sums(schwz_subdomain *sd, schwz_coarse *c, const double *d_vec, schwz_stream stream)
{
    SCHWZ_REQUIRE(sd && c && d_vec, "schwz_ras_aggregate_sums: null argument");
    SCHWZ_REQUIRE(sd->dev && sd->dev->coarse,
                  "schwz_ras_aggregate_sums: the subdomain has no aggregates (schwz_ras_coarse_set_aggregates)");
    schwz_coarse_part *p = sd->dev->coarse;
    SCHWZ_REQUIRE(c->nc == p->nc, "schwz_ras_aggregate_sums: the coarse object has another number of aggregates");
    if (p->m == 0) return SCHWZ_OK;
    hipStream_t st = (hipStream_t)stream;
    const int rc = ensure_agg_rows(sd, st);
    if (rc) return rc;
    if (p->nrow_pieces > 0) {
        hipLaunchKernelGGL(agg_partial_kernel, dim3(p->nrow_pieces), dim3(kBlock), 0, st, (const int32_t *)p->row_piece,
                           (const int32_t *)p->agg_rows, d_vec, (double *)p->row_partial);
        SCHWZ_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(agg_fold_kernel, dim3((p->m + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (int)p->m,
                       (const int32_t *)p->row_piece_ptr, (const double *)p->row_partial, (double *)c->s + p->first_agg);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

}  // extern "C"
