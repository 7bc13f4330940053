// Mixed-precision local solve (schwz_pcg_f32): preconditioned CG in fp32 on the fp64 start residual.
//
//   r0 = b - A x in fp64 through the matrix's best fp64 coding, nu = ||r0||_2
//   PCG on A32 e = r^ with r^ = fl32(r0 / nu), e0 = 0: fp32 matrix values and vectors, every dot product and norm
//   accumulated in fp64, the scalars (alpha, beta, rho) kept in fp64 and rounded when applied
//   x += nu e in fp64
//
// i.e. one step of iterative refinement; the RAS iteration, which recomputes b~ and the local residual in fp64
// every outer iteration and warm-starts the local solve, is the refinement loop.  A plain-CSR iteration streams
// 8 B per nonzero and 4 B per vector entry instead of 12 B and 8 B.
//
// Launches of one iteration (three): q = A32 p with the partial sums of p.q; e += alpha p, r -= alpha q with the
// partial sums of r.z and r.r; p = z + beta p (the last iteration of a solve: the state advance alone).  As in cg.hip
// the partial sums are one fp64 value per workgroup in grids of at most kMaxGrid workgroups, and every workgroup of
// the NEXT launch folds them itself in a fixed order (fold_partials): nothing is handed between workgroups inside a
// launch, there is no fence, no atomic, and the same input gives the same bits.  (A first version let the workgroup
// that arrived last at a ticket counter fold the sums of grids of any size: its release fence per workgroup and the
// adds on one word cost 3.6 ms per iteration at 256^3, profiles/r11_mixed_precision.txt.)  Scalars and the stop
// decision live in CgStateF32 in HBM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

#include "schwz_internal.hpp"
#include "device_utils.hpp"
#include "stream_pipeline.hpp"

namespace schwz {

constexpr int kSeq32 = 3;  // consecutive tiles per short-lived workgroup of the stream kernel (spmv_stream.hip)

struct CgStateF32 {
    double rho[2];
    double rr;   // ||r||^2 of the recurred (scaled) residual
    double r0;   // ||r^||_2
    double pq;   // written by schwz_pcg_f32_spmv only (the iteration folds the partial sums where it needs them)
    double nu;   // ||b - A x||_2
    int iters;
    int stop_iter;
};

// ---- fp32 copy of the matrix values ---------------------------------------------------------------------------

// val32[j] = fl32(val[j]), round to nearest; *bad = smallest j whose finite value rounds to +-inf
__global__ __launch_bounds__(kBlock) void f32_convert_kernel(int64_t nnz, const double *__restrict__ val,
                                                             float *__restrict__ val32, unsigned long long *bad)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < nnz; j += stride) {
        const double v = val[j];
        const float f = (float)v;
        val32[j] = f;
        if (isfinite(v) && isinf(f)) atomicMin(bad, (unsigned long long)j);
    }
}

// dinv32[i] = fl32(1 / A[i][i]) (1 where the row stores no diagonal)
__global__ __launch_bounds__(kBlock) void f32_dinv_kernel(CsrView A, float *__restrict__ dinv)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.nrows; i += stride) {
        double d = 1.0;
        for (int j = A.rp[i]; j < A.rp[i + 1]; ++j)
            if (A.col[j] == i) d = A.val[j];
        dinv[i] = (float)(1.0 / d);
    }
}

// ---- q = A32 p with the partial sums of p.q ---------------------------------------------------------------------

// The tile pipeline of stream_pipeline.hpp on fp32 values: one 16-byte load of 4 values and one of 4 columns per lane
// and half tile, 16 KiB of LDS per tile, q stored non-temporally.  seq > 0: short-lived workgroups, seq == 0:
// persistent ones (pcg_f32_build chooses).  Row sums are fp32; p_i q_i is added up in fp64, one partial sum per
// workgroup in part[blockIdx.x].
template <int CAP>
__global__ __launch_bounds__(kBlock) void f32_spmv_stream_kernel(CsrView A, const float *__restrict__ val32,
                                                                 const float *__restrict__ p, float *__restrict__ q,
                                                                 const CgStateF32 *st, int it, double *part, int seq)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const int tid = threadIdx.x;
    double acc = 0.0;
    // the own-row operand: p at the lane's row (p captured by value: read through a reference the load is no longer
    // known not to alias the q stores, which costs two registers and, at CAP = 8, a wave per SIMD)
    auto load = [p](int rowc) -> float { return p[rowc]; };
    auto row = [&](float sum, float pi, int rowc, bool mine) {
        __builtin_nontemporal_store(sum, q + rowc);
        const double t = (double)pi * (double)sum;
        acc += mine ? t : 0.0;
    };
    SCHWZ_STREAM_PIPELINE(A, CAP, float, val32, p, seq, true, float, load, row)
    const double s0 = block_sum(acc, red);
    if (tid == 0) part[blockIdx.x] = s0;
}

// Every other matrix (a row longer than 32 entries, a tile that does not fit the aligned window): one row per lane,
// summed in CSR order, grid-stride.  Built for correctness only.
__global__ __launch_bounds__(kBlock) void f32_spmv_rows_kernel(CsrView A, const float *__restrict__ val32,
                                                               const float *__restrict__ p, float *__restrict__ q,
                                                               const CgStateF32 *st, int it, double *part)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.nrows; i += stride) {
        float sum = 0.0f;
        for (int j = A.rp[i]; j < A.rp[i + 1]; ++j) sum += val32[j] * p[A.col[j]];
        q[i] = sum;
        acc += (double)p[i] * (double)sum;
    }
    const double s0 = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s0;
}

// ---- vector launches --------------------------------------------------------------------------------------------
// One 16-byte quad per lane and trip, grid-stride in at most kMaxGrid workgroups; the n % 4 tail elements are lane
// 0's of workgroup 0.  Partial sums: bank 0 at part[blockIdx.x], bank 1 at part[gridDim.x + blockIdx.x].

// partial sums of ||b - y||^2 (y = A x in fp64)
__global__ __launch_bounds__(kBlock) void f32_norm_kernel(int64_t n, const double *__restrict__ b,
                                                          const double *__restrict__ y, double *part)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double r = b[i] - y[i];
        acc += r * r;
    }
    const double s0 = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s0;
}

// r^ = fl32((b - y) / nu), z = D^-1 r^, p = z, e = 0; partial sums of r^.z and ||r^||^2.  nu from the partial sums of
// f32_norm_kernel; nu == 0: nothing is written but zero partial sums
__global__ __launch_bounds__(kBlock) void f32_entry_kernel(int64_t n, const double *__restrict__ b,
                                                           const double *__restrict__ y,
                                                           const float *__restrict__ dinv, float *__restrict__ r,
                                                           float *__restrict__ p, float *__restrict__ e,
                                                           const double *norm_part, int norm_nparts, double *part)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const double nu = sqrt(fold_partials(norm_part, norm_nparts, red));
    double a0 = 0.0, a1 = 0.0;
    if (nu != 0.0) {
        const int64_t nq = n >> 2, stride = (int64_t)gridDim.x * kBlock;
        for (int64_t iq = (int64_t)blockIdx.x * kBlock + threadIdx.x; iq < nq; iq += stride) {
            const int64_t i0 = 4 * iq;
            vf4 rv, zv;
#pragma unroll
            for (int u = 0; u < 4; ++u) rv[u] = (float)((b[i0 + u] - y[i0 + u]) / nu);
            zv = dinv ? *reinterpret_cast<const vf4 *>(dinv + i0) * rv : rv;
            *reinterpret_cast<vf4 *>(r + i0) = rv;
            *reinterpret_cast<vf4 *>(p + i0) = zv;
            *reinterpret_cast<vf4 *>(e + i0) = vf4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a0 += (double)rv[u] * (double)zv[u];
                a1 += (double)rv[u] * (double)rv[u];
            }
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int64_t i = 4 * nq; i < n; ++i) {
                const float rv = (float)((b[i] - y[i]) / nu);
                const float zv = dinv ? dinv[i] * rv : rv;
                r[i] = rv;
                p[i] = zv;
                e[i] = 0.0f;
                a0 += (double)rv * (double)zv;
                a1 += (double)rv * (double)rv;
            }
    }
    const double s0 = block_sum(a0, red);
    const double s1 = block_sum(a1, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s0;
        part[gridDim.x + blockIdx.x] = s1;
    }
}

// start of a solve: nu, rho, ||r^||^2 folded into the state (one workgroup)
__global__ __launch_bounds__(kBlock) void f32_init_state_kernel(CgStateF32 *st, const double *norm_part, int norm_nparts,
                                                                const double *part, int nparts, double rtol)
{
    __shared__ double red[4];
    const double nu = sqrt(fold_partials(norm_part, norm_nparts, red));
    const double rho = fold_partials(part, nparts, red);
    const double rr = fold_partials(part + nparts, nparts, red);
    if (threadIdx.x == 0) {
        st->nu = nu;
        st->rho[0] = rho;
        st->rho[1] = 0.0;
        st->rr = rr;
        st->r0 = sqrt(rr);
        st->pq = 0.0;
        st->iters = 0;
        // loop-top test of iteration 0, as cg_init_state has it; nu == 0 gives rr == 0: no iteration, x untouched
        st->stop_iter = (sqrt(rr) <= rtol * sqrt(rr)) ? 0 : INT_MAX;
    }
}

// e += alpha p ; r -= alpha q ; z = D^-1 r ; partial sums of r.z and r.r.  alpha from the partial sums of p.q
__global__ __launch_bounds__(kBlock) void f32_update_kernel(int64_t n, float *__restrict__ e, float *__restrict__ r,
                                                            const float *__restrict__ p, const float *__restrict__ q,
                                                            const float *__restrict__ dinv, const CgStateF32 *st, int it,
                                                            const double *pq_part, int pq_nparts, double *part)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const double pq = fold_partials(pq_part, pq_nparts, red);
    const float alpha = (float)(st->rho[it & 1] / pq);
    double a0 = 0.0, a1 = 0.0;
    const int64_t nq = n >> 2, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t iq = (int64_t)blockIdx.x * kBlock + threadIdx.x; iq < nq; iq += stride) {
        const int64_t i0 = 4 * iq;
        vf4 ev = *reinterpret_cast<const vf4 *>(e + i0), rv = *reinterpret_cast<const vf4 *>(r + i0);
        const vf4 pv = *reinterpret_cast<const vf4 *>(p + i0), qv = *reinterpret_cast<const vf4 *>(q + i0);
        ev += alpha * pv;
        rv -= alpha * qv;
        const vf4 zv = dinv ? *reinterpret_cast<const vf4 *>(dinv + i0) * rv : rv;
        *reinterpret_cast<vf4 *>(e + i0) = ev;
        *reinterpret_cast<vf4 *>(r + i0) = rv;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a0 += (double)rv[u] * (double)zv[u];
            a1 += (double)rv[u] * (double)rv[u];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = 4 * nq; i < n; ++i) {
            e[i] += alpha * p[i];
            const float rv = r[i] - alpha * q[i];
            r[i] = rv;
            const float zv = dinv ? dinv[i] * rv : rv;
            a0 += (double)rv * (double)zv;
            a1 += (double)rv * (double)rv;
        }
    const double s0 = block_sum(a0, red);
    const double s1 = block_sum(a1, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s0;
        part[gridDim.x + blockIdx.x] = s1;
    }
}

// p = D^-1 r + beta p, beta from the partial sums of the update launch; workgroup 0 advances the state.
// DIR = false: the state advance alone, one workgroup (the last iteration of a solve: nobody reads its direction)
template <bool DIR>
__global__ __launch_bounds__(kBlock) void f32_direction_kernel(int64_t n, float *__restrict__ p,
                                                               const float *__restrict__ r,
                                                               const float *__restrict__ dinv, CgStateF32 *st, int it,
                                                               double rtol, const double *part, int nparts)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const double rho_new = fold_partials(part, nparts, red);
    const double rr = fold_partials(part + nparts, nparts, red);
    if (DIR) {
        const float beta = (float)(rho_new / st->rho[it & 1]);
        const int64_t nq = n >> 2, stride = (int64_t)gridDim.x * kBlock;
        for (int64_t iq = (int64_t)blockIdx.x * kBlock + threadIdx.x; iq < nq; iq += stride) {
            const int64_t i0 = 4 * iq;
            const vf4 rv = *reinterpret_cast<const vf4 *>(r + i0), pv = *reinterpret_cast<const vf4 *>(p + i0);
            const vf4 zv = dinv ? *reinterpret_cast<const vf4 *>(dinv + i0) * rv : rv;
            *reinterpret_cast<vf4 *>(p + i0) = zv + beta * pv;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int64_t i = 4 * nq; i < n; ++i) {
                const float zv = dinv ? dinv[i] * r[i] : r[i];
                p[i] = zv + beta * p[i];
            }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // other workgroups read rho[it & 1] concurrently: the slot written here is the other one.  stop_iter = 0:
        // every later launch leaves at once; workgroups of THIS launch that read it early skip their part of p,
        // which nobody reads any more (as in cg_direction_kernel)
        st->rho[(it + 1) & 1] = rho_new;
        st->rr = rr;
        st->iters = st->iters + 1;
        if (sqrt(rr) <= rtol * st->r0) st->stop_iter = 0;
    }
}

// x += nu e in fp64 (nothing where no iteration was carried out: x keeps its bits)
__global__ __launch_bounds__(kBlock) void f32_exit_kernel(int64_t n, double *__restrict__ x,
                                                          const float *__restrict__ e, const CgStateF32 *st)
{
#pragma clang fp contract(off)
    if (st->iters == 0) return;
    const double nu = st->nu;
    typedef double vd2 __attribute__((ext_vector_type(2)));
    const int64_t nq = n >> 2, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t iq = (int64_t)blockIdx.x * kBlock + threadIdx.x; iq < nq; iq += stride) {
        const int64_t i0 = 4 * iq;
        const vf4 ev = *reinterpret_cast<const vf4 *>(e + i0);
        vd2 x0 = *reinterpret_cast<const vd2 *>(x + i0), x1 = *reinterpret_cast<const vd2 *>(x + i0 + 2);
        x0.x += nu * (double)ev[0];
        x0.y += nu * (double)ev[1];
        x1.x += nu * (double)ev[2];
        x1.y += nu * (double)ev[3];
        *reinterpret_cast<vd2 *>(x + i0) = x0;
        *reinterpret_cast<vd2 *>(x + i0 + 2) = x1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = 4 * nq; i < n; ++i) x[i] += nu * (double)e[i];
}

// schwz_pcg_f32_spmv: p.q folded as the update launch folds it
__global__ __launch_bounds__(kBlock) void f32_fold_pq_kernel(CgStateF32 *st, const double *part, int nparts)
{
    __shared__ double red[4];
    const double pq = fold_partials(part, nparts, red);
    if (threadIdx.x == 0) st->pq = pq;
}

}  // namespace schwz

using namespace schwz;

struct schwz_pcg_f32 {
    const schwz_csr *A = nullptr;
    int precond = 0;
    int64_t n = 0;
    Dev<float> val32;  // nnz + 4 (the 16-byte loads of a tile's last quad may touch the padding)
    Dev<float> r, p, q, e, dinv;
    Dev<double> y;     // A x of the start residual
    Dev<double> part;  // 4 banks of kMaxGrid partial sums: ||b - A x||^2, p.q, and r.z with r.r
    StateMirror<CgStateF32> state;
    int gs = 0, gv = 0;  // grids of the SpMV launch and of the vector launches, both <= kMaxGrid
    int seq = 0;         // tiles per short-lived workgroup of the stream kernel; 0: persistent workgroups
    double *part_norm() const { return part; }
    double *part_pq() const { return part + kMaxGrid; }
    double *part_vec() const { return part + 2 * kMaxGrid; }
};

// schwz_ras_restart: the state of the last solve (what schwz_pcg_f32_last_stats reports) back to zeros, as created
int schwz::pcg_f32_forget(schwz_pcg_f32 *s, hipStream_t st) { return s ? s->state.reset(st) : SCHWZ_OK; }

static int pcg_f32_build(schwz_pcg_f32 *s)
{
    const CsrView &A = s->A->v;
    const int64_t n = s->n, nnz = A.nnz;
    const size_t nv = (size_t)n + 4;  // entries of a vector
    // Every grid holds at most kMaxGrid workgroups, so that the workgroups of the next launch can fold its partial
    // sums themselves.  Vector launches: one quad per lane up to 4 * kBlock * kMaxGrid = 2 M entries, grid-stride
    // beyond.  Stream kernel: short-lived workgroups of kSeq32 consecutive tiles while such a grid fits (up to
    // 6144 tiles, about 1.5 M rows), persistent workgroups striding through their XCD's sequence beyond.
    s->gv = grid_for((n + 3) / 4);
    if (stream_takes(A)) {
        const int g = kXcds * ((stream_slots(A) + kSeq32 - 1) / kSeq32);
        s->seq = g <= kMaxGrid ? kSeq32 : 0;
        s->gs = s->seq ? g : kMaxGrid;
    } else {
        s->gs = grid_for(n);
    }
    int rc;
    if ((rc = s->val32.alloc((size_t)nnz + 4, true))) return rc;
    for (Dev<float> *v : {&s->r, &s->p, &s->q, &s->e})
        if ((rc = v->alloc(nv, true))) return rc;
    if ((rc = s->y.alloc((size_t)n)) || (rc = s->part.alloc((size_t)4 * kMaxGrid)) || (rc = s->state.create())) return rc;
    // the fp32 values, and whether every finite one stayed finite (read once, here)
    Dev<unsigned long long> d_bad;
    if ((rc = d_bad.alloc(1))) return rc;
    unsigned long long bad = ~0ull;
    SCHWZ_HIP_TRY(hipMemcpy(d_bad, &bad, sizeof(bad), hipMemcpyHostToDevice));
    if (nnz > 0) {
        hipLaunchKernelGGL(f32_convert_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, 0, nnz, A.val, s->val32, d_bad);
        SCHWZ_HIP_TRY(hipGetLastError());
    }
    SCHWZ_HIP_TRY(hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
    if (bad != ~0ull) {
        // name the entry: its row from the row pointers (error path only)
        std::vector<schwz_idx> rp((size_t)n + 1);
        schwz_idx c = 0;
        double v = 0.0;
        SCHWZ_HIP_TRY(hipMemcpy(rp.data(), A.rp, rp.size() * sizeof(schwz_idx), hipMemcpyDeviceToHost));
        SCHWZ_HIP_TRY(hipMemcpy(&c, A.col + bad, sizeof(c), hipMemcpyDeviceToHost));
        SCHWZ_HIP_TRY(hipMemcpy(&v, A.val + bad, sizeof(v), hipMemcpyDeviceToHost));
        const int64_t row = (int64_t)(std::upper_bound(rp.begin(), rp.end(), (schwz_idx)bad) - rp.begin()) - 1;
        char msg[200];
        std::snprintf(msg, sizeof(msg),
                      "schwz_pcg_f32_create: entry (%lld, %d) = %.17g of the matrix is not representable in fp32",
                      (long long)row, (int)c, v);
        set_error(msg);
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    if (s->precond == SCHWZ_PRECOND_JACOBI) {
        if ((rc = s->dinv.alloc(nv, true))) return rc;
        if (n) {
            hipLaunchKernelGGL(f32_dinv_kernel, dim3(grid_for(n)), dim3(kBlock), 0, 0, A, s->dinv);
            SCHWZ_HIP_TRY(hipGetLastError());
        }
    }
    SCHWZ_HIP_TRY(hipDeviceSynchronize());
    return SCHWZ_OK;
}

// q = A32 p and the partial sums of p.q (part_pq, gs of them) of iteration `it`
static int launch_spmv_f32(schwz_pcg_f32 *s, const float *p, float *q, int it, hipStream_t st)
{
    const CsrView &A = s->A->v;
    if (stream_takes(A)) {
        stream_cap_dispatch(A, [&](auto cap) {
            hipLaunchKernelGGL((f32_spmv_stream_kernel<decltype(cap)::value>), dim3(s->gs), dim3(kBlock), 0, st, A,
                               (const float *)s->val32, p, q, (const CgStateF32 *)s->state.dev(), it, s->part_pq(), s->seq);
        });
    } else {
        hipLaunchKernelGGL(f32_spmv_rows_kernel, dim3(s->gs), dim3(kBlock), 0, st, A, (const float *)s->val32, p, q,
                           (const CgStateF32 *)s->state.dev(), it, s->part_pq());
    }
    return SCHWZ_OK;
}

extern "C" {

int schwz_pcg_f32_create(const schwz_csr *A, int precond, schwz_pcg_f32 **out)
{
    // the argument checks come before the matrix is looked at (they need no device)
    SCHWZ_REQUIRE(out, "schwz_pcg_f32_create: null output");
    *out = nullptr;
    SCHWZ_REQUIRE(precond >= SCHWZ_PRECOND_NONE && precond <= SCHWZ_PRECOND_ISAI,
                  "schwz_pcg_f32_create: unknown preconditioner");
    if (precond != SCHWZ_PRECOND_NONE && precond != SCHWZ_PRECOND_JACOBI) {
        set_error("schwz_pcg_f32_create: the fp32 local solve exists without a preconditioner and with scalar Jacobi only");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    SCHWZ_REQUIRE(A, "schwz_pcg_f32_create: null matrix");
    SCHWZ_REQUIRE(A->v.nrows == A->v.ncols, "schwz_pcg_f32_create: matrix not square");
    schwz_pcg_f32 *s = new schwz_pcg_f32();
    s->A = A;
    s->precond = precond;
    s->n = A->v.nrows;
    const int rc = pcg_f32_build(s);
    if (rc) {
        schwz_pcg_f32_destroy(s);
        return rc;
    }
    *out = s;
    return SCHWZ_OK;
}

void schwz_pcg_f32_destroy(schwz_pcg_f32 *s) { delete s; }

int schwz_pcg_f32_solve(schwz_pcg_f32 *s, const double *d_b, double *d_x, double rtol, int max_iters, int *h_iters,
                        double *h_resnorm, schwz_stream stream)
{
    SCHWZ_REQUIRE(s && d_b && d_x, "schwz_pcg_f32_solve: null argument");
    SCHWZ_REQUIRE(max_iters >= 0, "schwz_pcg_f32_solve: negative max_iters");
    SCHWZ_REQUIRE((reinterpret_cast<uintptr_t>(d_x) & 15) == 0, "schwz_pcg_f32_solve: x must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = s->n;
    if (n == 0) {
        if (h_iters) *h_iters = 0;
        if (h_resnorm) *h_resnorm = 0.0;
        return SCHWZ_OK;
    }
    // entry: y = A x in fp64 (the matrix's best coding), nu = ||b - y||, r^ = fl32((b - y) / nu)
    SpmvArgs a;
    a.x = d_x;
    a.y = s->y;
    int rc = launch_spmv(s->A->v, kSpmvPlain, a, 0, st);
    if (rc) return rc;
    const dim3 gv(s->gv), blk(kBlock);
    hipLaunchKernelGGL(f32_norm_kernel, gv, blk, 0, st, n, d_b, (const double *)s->y, s->part_norm());
    hipLaunchKernelGGL(f32_entry_kernel, gv, blk, 0, st, n, d_b, (const double *)s->y, (const float *)s->dinv, s->r,
                       s->p, s->e, (const double *)s->part_norm(), s->gv, s->part_vec());
    hipLaunchKernelGGL(f32_init_state_kernel, dim3(1), blk, 0, st, s->state.dev(), (const double *)s->part_norm(), s->gv,
                       (const double *)s->part_vec(), s->gv, rtol);
    SCHWZ_HIP_TRY(hipGetLastError());
    // the control flow of pcg_iterate: with a tolerance, growing chunks of iterations (ChunkSchedule) and a poll of
    // the pinned state copy one chunk behind; launches past the stop iteration return at once
    const bool poll = rtol > 0.0;
    ChunkSchedule chunks;
    int it = 0;
    bool stopped = false;
    s->state.begin();
    while (it < max_iters && !stopped) {
        const int end = chunks.end(it, max_iters, poll);
        for (; it < end; ++it) {
            if ((rc = launch_spmv_f32(s, s->p, s->q, it, st))) return rc;
            hipLaunchKernelGGL(f32_update_kernel, gv, blk, 0, st, n, s->e, s->r, (const float *)s->p,
                               (const float *)s->q, (const float *)s->dinv, (const CgStateF32 *)s->state.dev(), it,
                               (const double *)s->part_pq(), s->gs, s->part_vec());
            if (it + 1 < max_iters)
                hipLaunchKernelGGL(f32_direction_kernel<true>, gv, blk, 0, st, n, s->p, (const float *)s->r,
                                   (const float *)s->dinv, s->state.dev(), it, rtol, (const double *)s->part_vec(), s->gv);
            else  // (the last iteration's direction is read by nobody: the state advance alone)
                hipLaunchKernelGGL(f32_direction_kernel<false>, dim3(1), blk, 0, st, n, s->p, (const float *)s->r,
                                   (const float *)s->dinv, s->state.dev(), it, rtol, (const double *)s->part_vec(), s->gv);
        }
        SCHWZ_HIP_TRY(hipGetLastError());
        if (poll && it < max_iters) {
            if ((rc = s->state.poll(st, &stopped))) return rc;
            chunks.grow();
        }
    }
    if (max_iters > 0) {
        hipLaunchKernelGGL(f32_exit_kernel, gv, blk, 0, st, n, d_x, (const float *)s->e, (const CgStateF32 *)s->state.dev());
        SCHWZ_HIP_TRY(hipGetLastError());
    }
    if (h_iters || h_resnorm) {
        if ((rc = s->state.read(st))) return rc;
        const CgStateF32 &h = s->state.host(0);
        if (h_iters) *h_iters = h.iters;
        if (h_resnorm) *h_resnorm = h.nu * std::sqrt(h.rr);
    }
    return SCHWZ_OK;
}

int schwz_pcg_f32_spmv(schwz_pcg_f32 *s, const float *d_p, float *d_q, double *h_pq, schwz_stream stream)
{
    SCHWZ_REQUIRE(s && d_p && d_q, "schwz_pcg_f32_spmv: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (s->n == 0) {
        if (h_pq) *h_pq = 0.0;
        return SCHWZ_OK;
    }
    // a state no launch leaves early on
    CgStateF32 &h = s->state.host(0);
    h = CgStateF32();
    h.stop_iter = INT_MAX;
    SCHWZ_HIP_TRY(hipMemcpyAsync(s->state.dev(), &h, sizeof(CgStateF32), hipMemcpyHostToDevice, st));
    int rc = launch_spmv_f32(s, d_p, d_q, 0, st);
    if (rc) return rc;
    hipLaunchKernelGGL(f32_fold_pq_kernel, dim3(1), dim3(kBlock), 0, st, s->state.dev(), (const double *)s->part_pq(), s->gs);
    SCHWZ_HIP_TRY(hipGetLastError());
    if ((rc = s->state.read(st))) return rc;
    if (h_pq) *h_pq = h.pq;
    return SCHWZ_OK;
}

int schwz_pcg_f32_last_stats(schwz_pcg_f32 *s, int *h_iters, double *h_resnorm)
{
    SCHWZ_REQUIRE(s && h_iters && h_resnorm, "schwz_pcg_f32_last_stats: null argument");
    if (const int rc = s->state.read_blocking()) return rc;
    *h_iters = s->state.host(0).iters;
    *h_resnorm = s->state.host(0).nu * std::sqrt(s->state.host(0).rr);
    return SCHWZ_OK;
}

}  // extern "C"
