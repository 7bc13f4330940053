// Device-resident preconditioned CG: the fused vector kernels, the preconditioner applications
// (Jacobi, block-Jacobi, ILU(0) sweeps, ISAI products), the stored-q and the q-free iteration,
// hipGraph replay for small systems, and the profiling hooks of bench.py's roofline leg.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

#include "schwz_internal.hpp"
#include "device_utils.hpp"

namespace schwz {

// ---------------------------------------------------------------------------
// CG vector kernels.  One CG iteration = spmv_tiled_kernel<kSpmvDot> + these two.
// Scalars live in CgState in HBM; nothing returns to the host inside the loop.
// ---------------------------------------------------------------------------

__global__ void cg_init_finalize_kernel(CgState *st, const double *partials, int nparts, double rtol,
                                        double *norm_sq_out, int norm_bank)
{
    __shared__ double red[4];
    cg_init_state(st, partials, nparts, rtol, norm_sq_out, norm_bank, red);  // (device_utils.hpp)
}

// (vd2, store2, diag_pair, diag_one: device_utils.hpp, shared with bicgstab.hip)

// x += alpha p ; r -= alpha q ; z = dinv r ; partials: r.z and r.r
// U: 16-byte elements per lane in flight per trip; NT: non-temporal stores; NOX: x and p are not touched
// (deferred x update of the stored-q iteration: alpha goes to *alpha_out instead, see cg_flush_x_kernel)
template <int U, bool NT, bool NOX = false>
__global__ __launch_bounds__(kBlock) void cg_update_kernel(int64_t n, double *__restrict__ x,
                                                           double *__restrict__ r,
                                                           const double *__restrict__ p,
                                                           const double *__restrict__ q,
                                                           const DiagView dg,
                                                           const double *pq_partials, int nparts_in,
                                                           const CgState *st, int it,
                                                           double *partials_out, double *alpha_out = nullptr)
{
    __shared__ double red[4];
    __shared__ double ddict[256];
    if (it >= st->stop_iter) return;
    if (dg.mode == 2) {
        if (threadIdx.x < dg.ndict) ddict[threadIdx.x] = dg.dict[threadIdx.x];
        __syncthreads();
    }
    const double *__restrict__ dinv = dg.mode == 1 ? dg.full : nullptr;
    const uint16_t *dc2 = reinterpret_cast<const uint16_t *>(dg.code);
    const double pq = fold_partials(pq_partials, nparts_in, red);
    const double alpha = st->rho[it & 1] / pq;
    if (NOX && alpha_out && blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = alpha;
    double a0 = 0.0, a1 = 0.0;
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const vd2 *x2 = reinterpret_cast<const vd2 *>(x);
    const vd2 *r2 = reinterpret_cast<const vd2 *>(r);
    const vd2 *p2 = reinterpret_cast<const vd2 *>(p);
    const vd2 *q2 = reinterpret_cast<const vd2 *>(q);
    const vd2 *d2 = reinterpret_cast<const vd2 *>(dinv);
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n2; i0 += stride * U) {
        vd2 xv[U], rv[U], pv[U], qv[U], dv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                if (!NOX) {
                    xv[u] = x2[i];
                    pv[u] = p2[i];
                }
                rv[u] = r2[i];
                qv[u] = q2[i];
                dv[u] = diag_pair(dg, d2, dc2, ddict, i);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                if (!NOX) {
                    // one fused multiply-add per element, spelled out: cg_flush_x_kernel (fused = 1) repeats it
                    xv[u].x = __builtin_fma(alpha, pv[u].x, xv[u].x);
                    xv[u].y = __builtin_fma(alpha, pv[u].y, xv[u].y);
                    store2<NT>(x, i, xv[u]);
                }
                rv[u] -= alpha * qv[u];
                store2<NT>(r, i, rv[u]);
                vd2 z = rv[u];
                if (dg.mode) z *= dv[u];
                a0 += rv[u].x * z.x;
                a0 += rv[u].y * z.y;
                a1 += rv[u].x * rv[u].x;
                a1 += rv[u].y * rv[u].y;
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        if (!NOX) x[i] = __builtin_fma(alpha, p[i], x[i]);
        const double rv = r[i] - alpha * q[i];
        r[i] = rv;
        const double z = dg.mode ? diag_one(dg, ddict, i) * rv : rv;
        a0 += rv * z;
        a1 += rv * rv;
    }
    const double s0 = block_sum(a0, red);
    const double s1 = block_sum(a1, red);
    if (threadIdx.x == 0) {
        partials_out[blockIdx.x] = s0;
        partials_out[gridDim.x + blockIdx.x] = s1;
    }
}

// beta = rho'/rho ; p = dinv r + beta p ; state update by workgroup 0
template <int U, bool NT>
__global__ __launch_bounds__(kBlock) void cg_direction_kernel(int64_t n, double *p, const double *__restrict__ r,
                                                              const DiagView dg,
                                                              const double *partials_in, int nparts,
                                                              CgState *st, int it, double rtol, double *p_out = nullptr)
{
    // p_out: the new direction goes to another vector (the ring of the deferred x update); each
    // element is read and written by the same lane, so p_out == p (in place) is the default
    if (!p_out) p_out = p;
    // with a general preconditioner `r` is already z = M^-1 r and dg.mode is 0
    __shared__ double red[4];
    __shared__ double ddict[256];
    if (it >= st->stop_iter) return;
    if (dg.mode == 2) {
        if (threadIdx.x < dg.ndict) ddict[threadIdx.x] = dg.dict[threadIdx.x];
        __syncthreads();
    }
    const double *__restrict__ dinv = dg.mode == 1 ? dg.full : nullptr;
    const uint16_t *dc2 = reinterpret_cast<const uint16_t *>(dg.code);
    const double rho_new = fold_partials(partials_in, nparts, red);
    const double rr = fold_partials(partials_in + nparts, nparts, red);
    const double beta = rho_new / st->rho[it & 1];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const vd2 *p2 = reinterpret_cast<const vd2 *>(p);
    const vd2 *r2 = reinterpret_cast<const vd2 *>(r);
    const vd2 *d2 = reinterpret_cast<const vd2 *>(dinv);
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n2; i0 += stride * U) {
        vd2 pv[U], zv[U], dv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                pv[u] = p2[i];
                zv[u] = r2[i];
                dv[u] = diag_pair(dg, d2, dc2, ddict, i);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n2) {
                if (dg.mode) zv[u] *= dv[u];
                store2<NT>(p_out, i, zv[u] + beta * pv[u]);
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double z = dg.mode ? diag_one(dg, ddict, i) * r[i] : r[i];
        p_out[i] = z + beta * p[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cg_advance_state(st, it, rho_new, rr, rtol);
}

// What workgroup 0 of cg_direction_kernel does, alone: the LAST iteration of a solve needs the state
// (rho, ||r||^2, the iteration count the deferred x update goes by) but no new search direction --
// 24 n bytes and 0.067 ms at 256^3 that nobody reads.
__global__ __launch_bounds__(kBlock) void cg_state_advance_kernel(const double *partials_in, int nparts, CgState *st,
                                                                   int it, double rtol)
{
    __shared__ double red[4];
    if (it >= st->stop_iter) return;
    const double rho_new = fold_partials(partials_in, nparts, red);
    const double rr = fold_partials(partials_in + nparts, nparts, red);
    if (threadIdx.x == 0) cg_advance_state(st, it, rho_new, rr, rtol);
}

// The last direction of a fixed-work solve is never stored (pcg_iterate, vlast_on): when somebody asks for the
// statistics of the postponed last iteration after all, its update launch needs that direction in memory --
// p = fma(beta, p_prev, D^-1 r), what the fused direction launch computed (the same operations: the same bits).
__global__ __launch_bounds__(kBlock) void cg_rebuild_direction_kernel(int64_t n, const double *__restrict__ p_prev,
                                                                      double prev_scale, const double *__restrict__ r,
                                                                      int dmode, double dsc, const CgState *st, int it,
                                                                      double *__restrict__ p_out)
{
#pragma clang fp contract(off)
    const double beta = st->rho[it & 1] / st->rho[(it - 1) & 1];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double pp = prev_scale * p_prev[i];
        const double zv = dmode ? dsc * r[i] : r[i];
        p_out[i] = __builtin_fma(beta, pp, zv);
    }
}

// Measured on MI355X (256^3): U = 2/4 and non-temporal stores change the PCG iteration time by
// < 1 % (0.403 / 0.406 / 0.417 ms for U = 1 / 2 / 4): these kernels sit at the mixed
// read+write HBM ceiling (~5.0-5.5 TB/s), so the plain shape is used.


// Deferred x update: x_i += alpha_k p_k,i for the iterations b0 <= k < b0 + count that were actually
// carried out, in iteration order and with the product rounded before the sum -- the very
// operations kSpmvCgUpdate performs when it updates x itself, so the bits are the same.
// Carried out: k < st->iters (the direction launch counts), plus iteration `pending` when this
// launch sits between its update launch and its direction launch and the update launch ran
// (pending < stop_iter, which only direction launches lower).
struct PRing {
    const double *slot[kDeferDepth];
};

// what every cg_flush_x_kernel launch of a solve is given alike (filled once per solve)
struct FlushX {
    int64_t n = 0;
    double *x = nullptr;                  // where x is stored (and, in place, read)
    PRing ring;
    const double *alpha_hist = nullptr;
    const CgState *st = nullptr;
    int fused = 0;                        // 1: x = fma(alpha, p, x) (stored-q iteration), 0: product rounded, then added
    const double *pq_partials = nullptr;  // lazy_it: the partial sums of p.(A p) its update launch would have folded
    int pq_nparts = 0;
    const double *x2_src = nullptr;       // rows [x2_rows, x2_total) of x2 are copied from here
    int64_t x2_total = 0;
    double p0_scale = 1.0;
    int dmode = 0;                        // vlast_it: D^-1 of the rebuilt direction (0: none, else the scalar dsc)
    double dsc = 1.0;
};

// ... and what differs between them: what only the launches that finish x carry, and x_in
struct FlushXLast {
    int lazy_it = -1, vlast_it = -1;
    const double *vlast_r = nullptr;  // the current residual
    double *x2 = nullptr;             // second output, rows [0, x2_rows)
    int64_t x2_rows = 0;
    const double *x_in = nullptr;     // out-of-place form (OOP): x is read from here and stored to FlushX::x
};

// The launch covers the pairs [pair0, pair1) (and the odd last row when `tail` is set): the last update of a
// solve is cut into the caller's priority rows and the rest (schwz_pcg::prio_*).
// lazy_it >= 0: the update launch of iteration lazy_it was not run (schwz_pcg::LazyLast); its direction counts
// as carried out and its alpha = rho / (p.Ap) is formed here from the partial sums that launch would have folded
// (the same expression, the same bits).  x2: rows [0, x2_rows) of the result are stored there as well (the
// restricted write-back of the RAS step) and the rows [x2_rows, x2_total) are copied from x2_src -- the overlap and
// halo entries of the current x~ --, so that x2 is the complete x~ after the restriction; with nothing to add the
// launch only copies.
// OOP, the out-of-place form (schwz_pcg::x_out): x is read from l.x_in, a vector the launch leaves untouched, and
// stored to f.x whether or not anything was added -- so f.x holds the whole of x after ONE such launch, and the
// later x updates of the solve run in place on it.  The arithmetic is the in-place form's.
template <bool OOP>
__global__ __launch_bounds__(kBlock) void cg_flush_x_kernel(const FlushX f, const FlushXLast l, int b0, int count,
                                                            int pending, int64_t pair0, int64_t pair1, int tail)
{
#pragma clang fp contract(off)
    // (the structs carry no qualifiers: the no-alias promises are made here)
    const int64_t n = f.n, x2_rows = l.x2_rows, x2_total = f.x2_total;
    double *__restrict__ const x = f.x;
    const double *__restrict__ const x_in = OOP ? l.x_in : nullptr;
    const PRing &ring = f.ring;
    const double *__restrict__ const alpha_hist = f.alpha_hist;
    const CgState *const st = f.st;
    const int fused = f.fused, lazy_it = l.lazy_it, pq_nparts = f.pq_nparts, vlast_it = l.vlast_it, vlast_dmode = f.dmode;
    const double *const pq_partials = f.pq_partials;
    double *__restrict__ const x2 = l.x2;
    const double *__restrict__ const x2_src = f.x2_src;
    const double *__restrict__ const vlast_r = l.vlast_r;
    const double p0_scale = f.p0_scale, vlast_dsc = f.dsc;
    // p0_scale: direction 0 of the solve is p0_scale x (slot 0 of the ring) -- 1.0 for a stored p0 (the product is
    // exact), D^-1's uniform factor when slot 0 is r0 and p0 = D^-1 r0 was never stored (virtual first direction:
    // the same rounded product the first-direction launch formed)
    // vlast_it >= 0: the direction of iteration vlast_it (the last one of the solve) was never stored either: it is
    // p = fma(beta, p_prev, D^-1 r) with beta = rho_new / rho_old as the fused direction launch formed it (both rho
    // slots still hold those values: the update launch of that iteration is the postponed one), p_prev the
    // direction before it and r = vlast_r the current residual -- the same operations, the same bits.
    __shared__ double alpha[kDeferDepth];
    __shared__ double red[4];
    const int stop = st->stop_iter;
    int done = st->iters + ((pending >= 0 && pending < stop) ? 1 : 0);
    if (lazy_it >= 0 && lazy_it < stop && done <= lazy_it) done = lazy_it + 1;
    const int kmax = min(count, done - b0);
    if (kmax <= 0 && !x2 && !OOP) return;
    double lazy_alpha = 0.0;
    if (kmax > 0 && lazy_it >= b0 && lazy_it < b0 + kmax)  // workgroup-uniform
        lazy_alpha = st->rho[lazy_it & 1] / fold_partials(pq_partials, pq_nparts, red);
    if ((int)threadIdx.x < kmax)
        alpha[threadIdx.x] = (b0 + (int)threadIdx.x == lazy_it) ? lazy_alpha : alpha_hist[(b0 + threadIdx.x) % kDeferDepth];
    __syncthreads();
    const int64_t n2 = pair1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    vd2 *x2v = reinterpret_cast<vd2 *>(x);
    const bool vlast = vlast_it >= b0 && vlast_it < b0 + kmax;  // workgroup-uniform
    const double vbeta = vlast ? st->rho[vlast_it & 1] / st->rho[(vlast_it - 1) & 1] : 0.0;
    const double *const vprev_slot = ring.slot[(vlast_it + kDeferDepth - 1) % kDeferDepth];
    const double vprev_scale = vlast_it == 1 ? p0_scale : 1.0;
    for (int64_t i = pair0 + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n2; i += stride) {
        vd2 xv = __builtin_nontemporal_load(OOP ? reinterpret_cast<const vd2 *>(x_in) + i : x2v + i);
        vd2 carry = {0.0, 0.0};  // direction of the iteration before the current group of four
        for (int k0 = 0; k0 < kmax; k0 += 4) {
            vd2 pv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k0 + k < kmax) {
                    if (vlast && b0 + k0 + k == vlast_it) {
                        pv[k] = __builtin_nontemporal_load(reinterpret_cast<const vd2 *>(vlast_r) + i);
                    } else {
                        pv[k] = __builtin_nontemporal_load(reinterpret_cast<const vd2 *>(ring.slot[(b0 + k0 + k) % kDeferDepth]) + i);
                        if (b0 + k0 + k == 0) pv[k] = p0_scale * pv[k];
                    }
                }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k0 + k < kmax) {
                    if (vlast && b0 + k0 + k == vlast_it) {
                        vd2 pp;
                        if (k > 0)
                            pp = pv[k - 1];
                        else if (k0 > 0)
                            pp = carry;
                        else
                            pp = vprev_scale * __builtin_nontemporal_load(reinterpret_cast<const vd2 *>(vprev_slot) + i);
                        const vd2 dsc2 = {vlast_dsc, vlast_dsc};
                        const vd2 zv = vlast_dmode ? dsc2 * pv[k] : pv[k];
                        pv[k].x = __builtin_fma(vbeta, pp.x, zv.x);
                        pv[k].y = __builtin_fma(vbeta, pp.y, zv.y);
                    }
                    if (fused) {  // the stored-q iteration's update: x = fma(alpha, p, x)
                        xv.x = __builtin_fma(alpha[k0 + k], pv[k].x, xv.x);
                        xv.y = __builtin_fma(alpha[k0 + k], pv[k].y, xv.y);
                    } else {      // the q-free update launch: product rounded, then added
                        const vd2 inc = alpha[k0 + k] * pv[k];
                        xv = xv + inc;
                    }
                }
            carry = pv[3];
        }
        if (OOP || kmax > 0) __builtin_nontemporal_store(xv, x2v + i);
        if (x2) {
            if (2 * i + 1 < x2_rows) {
                __builtin_nontemporal_store(xv, reinterpret_cast<vd2 *>(x2) + i);
            } else {
                if (2 * i < x2_rows)
                    x2[2 * i] = xv.x;
                else if (2 * i < x2_total)
                    x2[2 * i] = x2_src[2 * i];
                if (2 * i + 1 < x2_total) x2[2 * i + 1] = x2_src[2 * i + 1];
            }
        }
    }
    // entries of x2 beyond the solve's vector (the halo of x~): copied by the launch that takes the tail
    if (x2 && tail)
        for (int64_t j = 2 * pair1 + (int64_t)blockIdx.x * kBlock + threadIdx.x; j < x2_total; j += stride)
            if (!((n & 1) && j == n - 1)) x2[j] = x2_src[j];
    if (tail && (n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double xv = OOP ? x_in[n - 1] : x[n - 1];
        double pprev = vlast ? vprev_scale * vprev_slot[n - 1] : 0.0;
        for (int k = 0; k < kmax; ++k) {
            double pk;
            if (vlast && b0 + k == vlast_it) {
                const double rv = vlast_r[n - 1];
                const double zv = vlast_dmode ? vlast_dsc * rv : rv;
                pk = __builtin_fma(vbeta, pprev, zv);
            } else {
                pk = ring.slot[(b0 + k) % kDeferDepth][n - 1];
                if (b0 + k == 0) pk = p0_scale * pk;
            }
            pprev = pk;
            if (fused) {
                xv = __builtin_fma(alpha[k], pk, xv);
            } else {
                const double inc = alpha[k] * pk;
                xv = xv + inc;
            }
        }
        if (OOP || kmax > 0) x[n - 1] = xv;
        if (x2) x2[n - 1] = n - 1 < x2_rows ? xv : x2_src[n - 1];
    }
}

// dinv[i] = 1 / A[i][i] (1 when the row stores no diagonal): scalar Jacobi, i.e.
// block-Jacobi with max_block_size 1
__global__ void extract_dinv_kernel(CsrView A, double *__restrict__ dinv)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.nrows; i += stride) {
        double d = 1.0;
        for (int j = A.rp[i]; j < A.rp[i + 1]; ++j)
            if (A.col[j] == i) d = A.val[j];
        dinv[i] = 1.0 / d;
    }
}

// ---- block-Jacobi apply and the vector pieces of the general preconditioned CG -------------

// z[i] = sum_j inv[blk_id[i / bs]][i % bs][j] * r[(i / bs) * bs + j]
__global__ __launch_bounds__(kBlock) void block_jacobi_apply_kernel(int64_t n, int bs,
                                                                    const schwz_idx *__restrict__ blk_id,
                                                                    const double *__restrict__ blk_inv,
                                                                    const double *__restrict__ r,
                                                                    double *__restrict__ z)
{
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int64_t b = i / bs, r0 = b * bs;
        const double *row = blk_inv + ((int64_t)blk_id[b] * bs + (i - r0)) * bs;
        double s = 0.0;
        for (int j = 0; j < bs && r0 + j < n; ++j) s += row[j] * r[r0 + j];
        z[i] = s;
    }
}

// the same for detected blocks of different sizes (supervariable agglomeration): block of the row, its
// first row and size from blk_ptr
__global__ __launch_bounds__(kBlock) void block_jacobi_var_apply_kernel(int64_t n, int bs,
                                                                        const schwz_idx *__restrict__ row_blk,
                                                                        const schwz_idx *__restrict__ blk_ptr,
                                                                        const schwz_idx *__restrict__ blk_id,
                                                                        const double *__restrict__ blk_inv,
                                                                        const double *__restrict__ r,
                                                                        double *__restrict__ z)
{
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int b = row_blk[i];
        const int64_t r0 = blk_ptr[b];
        const int k = blk_ptr[b + 1] - blk_ptr[b];
        const double *row = blk_inv + ((int64_t)blk_id[b] * bs + (i - r0)) * bs;
        double s = 0.0;
        for (int j = 0; j < k; ++j) s += row[j] * r[r0 + j];
        z[i] = s;
    }
}

// partial sums of r.z and r.r (banks 0 and 1), optionally p := z
__global__ __launch_bounds__(kBlock) void dot_rz_kernel(int64_t n, const double *__restrict__ r,
                                                        const double *__restrict__ z, double *__restrict__ p_out,
                                                        const CgState *st, int it, double *partials_out)
{
    __shared__ double red[4];
    if (st && it >= st->stop_iter) return;
    double a0 = 0.0, a1 = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double rv = r[i], zv = z[i];
        a0 += rv * zv;
        a1 += rv * rv;
        if (p_out) p_out[i] = zv;
    }
    const double s0 = block_sum(a0, red);
    const double s1 = block_sum(a1, red);
    if (threadIdx.x == 0) {
        partials_out[blockIdx.x] = s0;
        partials_out[gridDim.x + blockIdx.x] = s1;
    }
}

}  // namespace schwz

using namespace schwz;

// ---- environment switches: the two idioms in use --------------------------------

// "0" switches off what is on by default
static bool env_on(const char *name)
{
    const char *e = std::getenv(name);
    return !(e && e[0] == '0');
}

// integer mode with a default
static int env_mode(const char *name, int dflt)
{
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

// ---- profiling hooks (bench.py roofline leg) ------------------------------------
// HIP-event pairs around the SpMV and the update launch of every CG iteration, on the stream
// they are launched on.

namespace {
struct ProfState {
    bool on = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> kind;  // per event pair: 0 = the SpMV launch of a CG iteration, 1 = its update launch
    size_t used = 0;
    double total[2] = {0.0, 0.0};
    int64_t count[2] = {0, 0};
} g_prof;
}  // namespace

extern "C" {

int schwz_profile_begin(int capacity)
{
    SCHWZ_REQUIRE(capacity > 0, "schwz_profile_begin: capacity must be positive");
    while (g_prof.ev.size() < (size_t)2 * capacity) {
        hipEvent_t e;
        SCHWZ_HIP_TRY(hipEventCreate(&e));
        g_prof.ev.push_back(e);
    }
    g_prof.kind.assign((size_t)capacity, 0);
    g_prof.used = 0;
    g_prof.on = true;
    return SCHWZ_OK;
}

int schwz_profile_end(double *h_total_ms, int64_t *h_launches)
{
    SCHWZ_REQUIRE(h_total_ms && h_launches, "schwz_profile_end: null output");
    g_prof.on = false;
    SCHWZ_HIP_TRY(hipDeviceSynchronize());
    g_prof.total[0] = g_prof.total[1] = 0.0;
    g_prof.count[0] = g_prof.count[1] = 0;
    for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
        float ms = 0.f;
        SCHWZ_HIP_TRY(hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]));
        const int k = g_prof.kind[i / 2] ? 1 : 0;
        g_prof.total[k] += ms;
        g_prof.count[k] += 1;
    }
    *h_total_ms = g_prof.total[0];
    *h_launches = g_prof.count[0];
    g_prof.used = 0;
    return SCHWZ_OK;
}

int schwz_profile_kind(int kind, double *h_total_ms, int64_t *h_launches)
{
    SCHWZ_REQUIRE(h_total_ms && h_launches && (kind == 0 || kind == 1), "schwz_profile_kind: bad arguments");
    *h_total_ms = g_prof.total[kind];
    *h_launches = g_prof.count[kind];
    return SCHWZ_OK;
}

// ---- PCG --------------------------------------------------------------------

int schwz_pcg_flavour(const schwz_pcg *s) { return s ? s->last_flavour : 0; }

int schwz_pcg_create(const schwz_csr *A, int precond, schwz_pcg **out)
{
    return schwz_pcg_create_ex(A, precond, 1, out);
}

// block-Jacobi / ILU(0) setup: the (setup-time) host copy of the matrix comes back from HBM
static int pcg_setup_general(schwz_pcg *s)
{
    const CsrView &A = s->A->v;
    const int64_t n = s->n;
    std::vector<schwz_idx> rp((size_t)n + 1), col((size_t)A.nnz);
    // (ParILU reads the values in HBM: only the pattern comes back)
    std::vector<double> val(s->par_ilu_sweeps > 0 ? 0 : (size_t)A.nnz);
    SCHWZ_HIP_TRY(hipMemcpy(rp.data(), A.rp, rp.size() * sizeof(schwz_idx), hipMemcpyDeviceToHost));
    if (A.nnz) {
        SCHWZ_HIP_TRY(hipMemcpy(col.data(), A.col, col.size() * sizeof(schwz_idx), hipMemcpyDeviceToHost));
        if (!val.empty())
            SCHWZ_HIP_TRY(hipMemcpy(val.data(), A.val, val.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (const int rc_z = s->z.alloc((size_t)n)) return rc_z;
    if (s->precond == SCHWZ_PRECOND_ILU || s->precond == SCHWZ_PRECOND_ISAI) {
        schwz_idx *l_rp, *l_col, *u_rp, *u_col;
        double *l_val, *u_val;
        int rc;
        if (s->par_ilu_sweeps > 0) {
            // ParILU sweeps on the GPU over the matrix in HBM (csrc/parilu.hip); the factors come back once
            StageTimer timer_pi("pcg_create: ParILU factors");
            rc = parilu_host_factors(n, rp.data(), col.data(), A.val, s->par_ilu_sweeps, &l_rp, &l_col, &l_val, &u_rp,
                                     &u_col, &u_val);
        } else {
            StageTimer timer_ilu("pcg_create: host ILU(0)");
            rc = schwz_ilu0(n, rp.data(), col.data(), val.data(), &l_rp, &l_col, &l_val, &u_rp, &u_col, &u_val);
        }
        if (rc) return rc;
        if (s->precond == SCHWZ_PRECOND_ISAI) {
            // Ilu<LowerIsai, UpperIsai> (solve.cpp:616-638): z = W_U (W_L r), two CSR products on
            // the patterns of L and U, stored like any other matrix of this library
            double *wl = nullptr, *wu = nullptr;
            rc = schwz_isai(n, l_rp, l_col, l_val, 1, &wl);
            if (!rc) rc = schwz_isai(n, u_rp, u_col, u_val, 0, &wu);
            if (!rc) rc = schwz_csr_create(n, n, l_rp, l_col, wl, &s->isai_l);
            if (!rc) rc = schwz_csr_create(n, n, u_rp, u_col, wu, &s->isai_u);
            if (!rc) rc = s->isai_tmp.alloc((size_t)n);
            schwz_free(wl);
            schwz_free(wu);
        } else if (s->trisolve_sweeps > 0) {
            StageTimer timer_trs("pcg_create: Jacobi-sweep triangular solves");
            rc = schwz_trs_create_sweeps(n, l_rp, l_col, l_val, u_rp, u_col, u_val, s->trisolve_sweeps, &s->ilu);
        } else {
            StageTimer timer_trs("pcg_create: triangular-solve analysis");
            rc = schwz_trs_create(n, l_rp, l_col, l_val, u_rp, u_col, u_val, nullptr, &s->ilu);
        }
        schwz_free(l_rp);
        schwz_free(l_col);
        schwz_free(l_val);
        schwz_free(u_rp);
        schwz_free(u_col);
        schwz_free(u_val);
        return rc;
    }
    // block-Jacobi.  Blocks as gko::preconditioner::Jacobi finds them when only max_block_size is given
    // (solve.cpp:490-505; Ginkgo's published find_blocks = find_natural_blocks + agglomerate_supervariables,
    // restated in oracle/schwz_oracle.c::detect_jacobi_blocks): maximal runs of consecutive rows with the
    // same column pattern, cut at bs rows, then merged left to right while a merged block stays within bs
    // rows.  Stencil matrices get consecutive blocks of exactly bs rows.  Every block is inverted by
    // Gauss-Jordan with partial pivoting; identical inverse blocks are stored once.
    const int bs = s->block_size;
    std::vector<schwz_idx> bptr;
    bptr.push_back(0);
    if (n > 0) {
        std::vector<schwz_idx> nat;
        nat.push_back(0);
        schwz_idx cur = 1;
        for (int64_t i = 0; i + 1 < n; ++i) {
            const schwz_idx la = rp[(size_t)i + 1] - rp[(size_t)i], lb = rp[(size_t)i + 2] - rp[(size_t)i + 1];
            bool same = la == lb;
            for (schwz_idx k = 0; same && k < la; ++k) same = col[(size_t)(rp[(size_t)i] + k)] == col[(size_t)(rp[(size_t)i + 1] + k)];
            if (cur < bs && same) {
                ++cur;
            } else {
                nat.push_back(nat.back() + cur);
                cur = 1;
            }
        }
        nat.push_back(nat.back() + cur);
        cur = nat[1] - nat[0];
        for (size_t i = 1; i + 1 < nat.size(); ++i) {
            const schwz_idx size = nat[i + 1] - nat[i];
            if (cur + size <= bs) {
                cur += size;
            } else {
                bptr.push_back(bptr.back() + cur);
                cur = size;
            }
        }
        bptr.push_back(bptr.back() + cur);
    }
    const int64_t nb = (int64_t)bptr.size() - 1;
    bool uniform = true;
    for (int64_t b = 0; b < nb && uniform; ++b) uniform = bptr[(size_t)b] == b * bs;
    std::vector<schwz_idx> id((size_t)nb), row_blk;
    if (!uniform) row_blk.resize((size_t)n);
    std::vector<double> uniq, blk((size_t)bs * bs), inv((size_t)bs * bs), padded((size_t)bs * bs);
    std::unordered_multimap<uint64_t, schwz_idx> seen;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t r0 = bptr[(size_t)b];
        const int k = (int)(bptr[(size_t)b + 1] - r0);
        std::fill(blk.begin(), blk.end(), 0.0);
        for (int i = 0; i < k; ++i) {
            if (!uniform) row_blk[(size_t)(r0 + i)] = (schwz_idx)b;
            for (schwz_idx j = rp[(size_t)(r0 + i)]; j < rp[(size_t)(r0 + i) + 1]; ++j)
                if (col[(size_t)j] >= r0 && col[(size_t)j] < r0 + k)
                    blk[(size_t)i * k + (col[(size_t)j] - r0)] = val[(size_t)j];
        }
        // invert the k x k block (the copy in blk is destroyed)
        std::vector<double> &a = blk;
        for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) inv[(size_t)i * k + j] = i == j ? 1.0 : 0.0;
        for (int c = 0; c < k; ++c) {
            int piv = c;
            for (int r = c + 1; r < k; ++r)
                if (std::fabs(a[(size_t)r * k + c]) > std::fabs(a[(size_t)piv * k + c])) piv = r;
            if (a[(size_t)piv * k + c] == 0.0) {
                set_error("block-Jacobi: singular diagonal block");
                return SCHWZ_ERR_NOT_SPD;
            }
            if (piv != c)
                for (int j = 0; j < k; ++j) {
                    std::swap(a[(size_t)c * k + j], a[(size_t)piv * k + j]);
                    std::swap(inv[(size_t)c * k + j], inv[(size_t)piv * k + j]);
                }
            const double d = a[(size_t)c * k + c];
            for (int j = 0; j < k; ++j) {
                a[(size_t)c * k + j] /= d;
                inv[(size_t)c * k + j] /= d;
            }
            for (int r = 0; r < k; ++r) {
                if (r == c) continue;
                const double f = a[(size_t)r * k + c];
                if (f == 0.0) continue;
                for (int j = 0; j < k; ++j) {
                    a[(size_t)r * k + j] -= f * a[(size_t)c * k + j];
                    inv[(size_t)r * k + j] -= f * inv[(size_t)c * k + j];
                }
            }
        }
        // stored in the top left corner of a bs x bs slot
        std::fill(padded.begin(), padded.end(), 0.0);
        for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) padded[(size_t)i * bs + j] = inv[(size_t)i * k + j];
        uint64_t h = 1469598103934665603ull ^ (uint64_t)k;
        for (double v : padded) {
            uint64_t bits;
            std::memcpy(&bits, &v, 8);
            h = (h ^ bits) * 1099511628211ull;
        }
        schwz_idx found = -1;
        auto range = seen.equal_range(h);
        for (auto it = range.first; it != range.second; ++it)
            if (std::memcmp(&uniq[(size_t)it->second * bs * bs], padded.data(), sizeof(double) * bs * bs) == 0) {
                found = it->second;
                break;
            }
        if (found < 0) {
            found = (schwz_idx)(uniq.size() / ((size_t)bs * bs));
            uniq.insert(uniq.end(), padded.begin(), padded.end());
            seen.emplace(h, found);
        }
        id[(size_t)b] = found;
    }
    int rc;
    if ((rc = s->d_blk_id.put(id)) || (rc = s->d_blk_inv.put(uniq))) return rc;
    if (!uniform && ((rc = s->d_row_blk.put(row_blk)) || (rc = s->d_blk_ptr.put(bptr)))) return rc;
    return SCHWZ_OK;
}

// everything of schwz_pcg_create_ex that can fail half way: the caller destroys `s` on error
static int pcg_build(schwz_pcg *s, const schwz_csr *A, int precond)
{
    const size_t n = (size_t)s->n;
    int rc;
    if ((rc = s->r.alloc(n)) || (rc = s->p.alloc(n)) || (rc = s->q.alloc(n)) || (rc = s->partials.alloc(8 * kMaxGrid)))
        return rc;
    s->stream_part = stream_part_alloc(A->v);
    if ((rc = s->norm_sq_own.alloc(2)) || (rc = s->state.create())) return rc;
    s->d_norm_sq = s->norm_sq_own;
    if (precond == SCHWZ_PRECOND_JACOBI) {
        if ((rc = s->dinv.alloc(n))) return rc;
        if (s->n) {
            hipLaunchKernelGGL(extract_dinv_kernel, dim3(grid_for(s->n)), dim3(kBlock), 0, 0, A->v, s->dinv);
            SCHWZ_HIP_TRY(hipGetLastError());
            SCHWZ_HIP_TRY(hipDeviceSynchronize());
        }
        // compact representation for the per-iteration vector kernels (DiagView)
        s->diag.mode = 1;
        s->diag.full = s->dinv;
        if (s->n && env_on("SCHWZ_DIAG_DICT")) {
            std::vector<double> h((size_t)s->n);
            SCHWZ_HIP_TRY(hipMemcpy(h.data(), s->dinv, (size_t)s->n * sizeof(double), hipMemcpyDeviceToHost));
            std::vector<double> dict;
            std::vector<uint8_t> code((size_t)s->n + 2, 0);
            bool ok = true;
            for (int64_t i = 0; i < s->n && ok; ++i) {
                int c = -1;
                for (size_t k = 0; k < dict.size(); ++k)
                    if (std::memcmp(&dict[k], &h[(size_t)i], 8) == 0) {
                        c = (int)k;
                        break;
                    }
                if (c < 0) {
                    if (dict.size() == 256) {
                        ok = false;
                        break;
                    }
                    c = (int)dict.size();
                    dict.push_back(h[(size_t)i]);
                }
                code[(size_t)i] = (uint8_t)c;
            }
            if (ok && dict.size() == 1) {
                s->diag.mode = 3;
                s->diag.uniform = dict[0];
            } else if (ok && dict.size() <= 16 && !A->v.pair_id) {  // linear search above stays cheap
                // (row-pair coded matrices keep the full vector: their q-free iteration reads it as
                // such and beats the stored-q iteration the codes would select)
                if ((rc = s->d_dcode.put(code)) || (rc = s->d_ddict.put(dict))) return rc;
                s->diag.mode = 2;
                s->diag.code = s->d_dcode.as<uint8_t>();
                s->diag.dict = s->d_ddict.as<double>();
                s->diag.ndict = (int)dict.size();
            }
        }
    }
    if (precond == SCHWZ_PRECOND_BLOCK_JACOBI || precond == SCHWZ_PRECOND_ILU || precond == SCHWZ_PRECOND_ISAI) {
        if ((rc = pcg_setup_general(s))) return rc;
    }
    return SCHWZ_OK;
}

int schwz_pcg_create_ex(const schwz_csr *A, int precond, int block_size, schwz_pcg **out)
{
    return pcg_create_impl(A, precond, block_size, 0, 0, out);
}

int schwz_pcg_create_ilu(const schwz_csr *A, int precond, int par_ilu_sweeps, int trisolve_sweeps, schwz_pcg **out)
{
    const int rc = pcg_check_ilu_sweeps(precond, par_ilu_sweeps, trisolve_sweeps);
    if (rc) return rc;
    return pcg_create_impl(A, precond, 1, par_ilu_sweeps, trisolve_sweeps, out);
}

}  // extern "C"

int schwz::pcg_check_ilu_sweeps(int precond, int par_ilu_sweeps, int trisolve_sweeps)
{
    SCHWZ_REQUIRE(par_ilu_sweeps >= 0 && trisolve_sweeps >= 0, "par_ilu_sweeps / trisolve_sweeps must be >= 0");
    if (par_ilu_sweeps > 0 && precond != SCHWZ_PRECOND_ILU && precond != SCHWZ_PRECOND_ISAI) {
        set_error("par_ilu_sweeps applies to the ilu and isai preconditioners only");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    if (trisolve_sweeps > 0 && precond != SCHWZ_PRECOND_ILU) {
        set_error("trisolve_sweeps applies to the ilu preconditioner only");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    return SCHWZ_OK;
}

int schwz::pcg_create_impl(const schwz_csr *A, int precond, int block_size, int par_ilu_sweeps, int trisolve_sweeps,
                           schwz_pcg **out)
{
    StageTimer timer_all("pcg_create (diagonal, preconditioner data, vectors)");
    SCHWZ_REQUIRE(A && out, "schwz_pcg_create: null argument");
    SCHWZ_REQUIRE(A->v.nrows == A->v.ncols, "schwz_pcg_create: matrix not square");
    SCHWZ_REQUIRE(precond >= SCHWZ_PRECOND_NONE && precond <= SCHWZ_PRECOND_ISAI,
                  "schwz_pcg_create: unknown preconditioner");
    SCHWZ_REQUIRE(block_size >= 1 && block_size <= 32, "schwz_pcg_create: block size must be in 1..32");
    if (precond == SCHWZ_PRECOND_BLOCK_JACOBI && block_size == 1) precond = SCHWZ_PRECOND_JACOBI;
    schwz_pcg *s = new schwz_pcg();
    s->A = A;
    s->precond = precond;
    s->block_size = block_size;
    s->par_ilu_sweeps = par_ilu_sweeps;
    s->trisolve_sweeps = trisolve_sweeps;
    s->n = A->v.nrows;
    const int rc = pcg_build(s, A, precond);
    if (rc) {
        schwz_pcg_destroy(s);
        return rc;
    }
    *out = s;
    return SCHWZ_OK;
}

extern "C" {

// the adopted objects, then the solver: its buffers, events, streams and recorded graphs release themselves
void schwz_pcg_destroy(schwz_pcg *s)
{
    if (!s) return;
    schwz_trs_destroy(s->ilu);
    schwz_csr_destroy(s->isai_l);
    schwz_csr_destroy(s->isai_u);
    delete s;
}

}  // extern "C"

namespace schwz {

// z = M^-1 r for the preconditioners that are operators of their own
__global__ __launch_bounds__(kBlock) void diag_scale_kernel(int64_t n, const double *__restrict__ dinv,
                                                            const double *__restrict__ in, double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = dinv[i] * in[i];
}

// out = M^-1 in for whichever preconditioner the object holds (in != out)
int precond_apply(schwz_pcg *s, const double *in, double *out, hipStream_t st)
{
    if (s->n == 0) return SCHWZ_OK;
    if (s->precond == SCHWZ_PRECOND_ILU) return schwz_trs_solve(s->ilu, in, out, (schwz_stream)st);
    if (s->precond == SCHWZ_PRECOND_ISAI) {
        SpmvArgs a;
        a.x = in;
        a.y = s->isai_tmp;
        int rc = launch_spmv(s->isai_l->v, kSpmvPlain, a, 0, st);
        if (rc) return rc;
        a.x = s->isai_tmp;
        a.y = out;
        return launch_spmv(s->isai_u->v, kSpmvPlain, a, 0, st);
    }
    if (s->precond == SCHWZ_PRECOND_BLOCK_JACOBI && s->d_row_blk) {
        hipLaunchKernelGGL(block_jacobi_var_apply_kernel, dim3(grid_for(s->n)), dim3(kBlock), 0, st, s->n, s->block_size,
                           s->d_row_blk, s->d_blk_ptr, s->d_blk_id, s->d_blk_inv, in, out);
    } else if (s->precond == SCHWZ_PRECOND_BLOCK_JACOBI) {
        hipLaunchKernelGGL(block_jacobi_apply_kernel, dim3(grid_for(s->n)), dim3(kBlock), 0, st, s->n, s->block_size,
                           s->d_blk_id, s->d_blk_inv, in, out);
    } else if (s->precond == SCHWZ_PRECOND_JACOBI) {
        hipLaunchKernelGGL(diag_scale_kernel, dim3(grid_for(s->n)), dim3(kBlock), 0, st, s->n, s->dinv, in, out);
    } else {
        return launch_copy(s->n, in, out, st);
    }
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

static int pcg_apply_general(schwz_pcg *s, hipStream_t st) { return precond_apply(s, s->r, s->z, st); }

int pcg_take_trs_error(schwz_pcg *s) { return s && s->ilu ? trs_take_error(s->ilu) : SCHWZ_OK; }

// The residual update and state advance a solve postponed (schwz_pcg::LazyLast): launched now, on the solve's
// stream, for a caller that wants the iteration count or the final residual norm.
int pcg_finish_lazy(schwz_pcg *s)
{
    if (!s || !s->lazy.pending) return SCHWZ_OK;
    s->lazy.pending = false;
    return s->lazy_run ? s->lazy_run(s->lazy.stream) : SCHWZ_OK;
}

// Between two solves of a set-up subdomain (schwz_ras_restart): everything the object remembers of its last solve
// is forgotten, as after creation.  The postponed launches are DROPPED, never run -- they would update a residual of
// the old right-hand side -- and with them the saved stream handle; the second outputs belong to buffers the caller
// is about to rewrite; the device state goes back to zeros behind what `st` holds.  What follows from the matrix
// stays: the plan's buffers, the recorded graphs, the priority rows and their event.
int pcg_forget(schwz_pcg *s, hipStream_t st)
{
    if (!s) return SCHWZ_OK;
    s->lazy = schwz_pcg::LazyLast();
    s->lazy_run = nullptr;
    s->x2_written = false;
    s->x2_out = nullptr;
    s->x2_src = nullptr;
    s->x_out = nullptr;
    s->p_pending = false;
    s->init = schwz_pcg::InitFold();
    s->init_event = nullptr;
    s->last_flavour = 0;
    return s->state.reset(st);
}

int pcg_last_stats(schwz_pcg *s, int *h_iters, double *h_resnorm)
{
    const int rc_lazy = pcg_finish_lazy(s);
    if (rc_lazy) return rc_lazy;
    if (const int rc = s->state.read_blocking()) return rc;
    *h_iters = s->state.host(0).iters;
    *h_resnorm = sqrt(s->state.host(0).rr);
    if (*h_resnorm != *h_resnorm) return pcg_take_trs_error(s);
    return SCHWZ_OK;
}

static bool pcg_is_general(const schwz_pcg *s)
{
    return s->precond == SCHWZ_PRECOND_BLOCK_JACOBI || s->precond == SCHWZ_PRECOND_ILU ||
           s->precond == SCHWZ_PRECOND_ISAI;
}

// ---- the plan of a solve (CgPlan, schwz_internal.hpp) -----------------------------------------------------------
// Every SCHWZ_CG_* switch is read here (env_on / env_mode), each in one place, and nowhere else.

// What follows from the matrix, the preconditioner and the switches: decided once per solve, by pcg_begin, which
// keeps it for pcg_iterate.  It only decides -- the buffers the plan needs are pcg_acquire_buffers' business.
static CgPlan pcg_plan_matrix(const schwz_pcg *s)
{
    CgPlan pl;
    const CsrView &A = s->A->v;
    const int64_t n = s->n;
    const int dmode = s->diag.mode;
    pl.gs = spmv_grid(A, s->variant);
    pl.gv = grid_for((n + 1) / 2);
    pl.general = pcg_is_general(s);
    // SCHWZ_CG_QFREE=0 keeps the stored-q iteration for row-pair coded matrices too (A/B runs)
    static const bool qfree_on = env_on("SCHWZ_CG_QFREE");
    pl.qfree = qfree_on && !pl.general && A.pair_id && s->variant == 0 && dmode != 2;
    // p.(A p) from the upper triangle when the upload found the matrix symmetric (SCHWZ_CG_SYM=0: full rows)
    static const bool sym_on = env_on("SCHWZ_CG_SYM");
    pl.dot_mode = !pl.qfree ? kSpmvDot : (sym_on && A.pair_sym_base > 0 ? kSpmvDotSym : kSpmvDotOnly);
    // Two launches per iteration: the direction update and the NEXT iteration's p.(A p) share one
    // launch (kSpmvDirDotSym), p alternating between two buffers (a launch that recomputes its
    // neighbours' new p must not overwrite the old one): s->p and the otherwise unused s->q, or the
    // slots of the deferred-x ring.  The first p.(A p) of a solve is launched on its own.
    // On launch-bound systems (up to kGraphRows rows) this is -11 to -13 % per outer iteration.  On
    // large ones the fused launch costs what the two it replaces cost -- 0.102 vs 0.067 + 0.045 ms on the
    // 256^3 cube (+1 % on the bench line), 0.111 vs 0.067 + 0.043 ms on the 512 x 512 x 64 slab of the
    // multi-GPU runs (-1 %) -- so they keep three launches.  SCHWZ_CG_FUSEDIR=0: never, =2: every size
    // (it combines with the deferred x update).
    static const int fusedir_mode = env_mode("SCHWZ_CG_FUSEDIR", 1);
    // ... unless the matrix takes the z-sweep walk (spmv_pair.hip, which owns the conditions): there the fused
    // launch loads every element of r and p once instead of gathering both at every entry, and replaces 32 n
    // bytes of the two launches by 24 n (SCHWZ_CG_SWEEP=0: chunk-by-chunk launches only; read per solve: tests
    // switch it, like the other switches that are not static here).
    pl.sweep_on = env_on("SCHWZ_CG_SWEEP") && s->variant == 0 && pair_sweep_update_ok(A, pl.gs, dmode);
    pl.sweep_dirdot = pl.sweep_on && pair_sweep_dirdot_ok(A, pl.gs, dmode);
    pl.fusedir = pl.dot_mode == kSpmvDotSym &&
                 (fusedir_mode == 2 || (fusedir_mode == 1 && (n <= kGraphRows || pl.sweep_dirdot)));
    // Large systems: x is not touched inside the iteration.  The search directions of up to
    // kDeferDepth iterations stay in a ring (slots 0 and 1 are s->p and the otherwise unused s->q),
    // the update launch stores alpha_k instead of updating x, and one launch per kDeferDepth
    // iterations (and one at the end) applies x += sum_k alpha_k p_k in iteration order -- the same
    // bits, (depth + 2) / depth vectors of traffic per iteration instead of 2.
    // SCHWZ_CG_DEFERX=0: never, =2: every size (tests).
    // The stored-q iteration of the scalar-Jacobi / unpreconditioned CG (plain CSR and the other codings)
    // defers x the same way; its ring cannot use s->q (it holds q), so it takes one more vector.
    const int dx_mode = env_mode("SCHWZ_CG_DEFERX", 1);
    pl.deferx = !pl.general && !s->ring_failed && (dx_mode == 2 || (dx_mode == 1 && n > kGraphRows));
    // A solve whose iterations all run in the walk starts in it as well: the start launch takes the walk
    // (32 n -> 24 n bytes: p is not stored) and the first p.(A p) comes from the FIRST form of the fused
    // direction launch, which builds p = D^-1 r from the r it reads anyway (SCHWZ_CG_SWEEPSTART=0: the
    // chunk-by-chunk start launch + kSpmvDotSym).
    pl.sweep_start = env_on("SCHWZ_CG_SWEEPSTART") && pl.deferx && pl.sweep_dirdot && pl.fusedir &&
                     pair_sweep_start_ok(A, pl.gs);
    // A start in the walk leaves the partial sums of rho, ||r||^2 and the check norm to workgroup 0 of the
    // first-direction launch, which folds them into CgState behind its first window requests -- the separate
    // one-workgroup launch between two full-grid ones (8 us and a launch boundary at 256^3) is gone, the same
    // folds in the same order (cg_init_state).  SCHWZ_CG_INITFOLD=0: cg_init_finalize_kernel as for every other start.
    pl.initfold = env_on("SCHWZ_CG_INITFOLD");
    return pl;
}

// What depends on rtol, max_iters and on whether the start launch left p pending: pcg_iterate, on its copy.
static void pcg_plan_solve(const schwz_pcg *s, CgPlan &pl, double rtol, int max_iters)
{
    // the walks serve every launch of the solve, and D^-1 is a scalar or absent
    const bool all_walks = pl.fusedir && pl.sweep_start && pl.sweep_on && pl.sweep_dirdot && pl.qfree &&
                           (s->diag.mode == 0 || s->diag.mode == 3);
    pl.walk_started = s->p_pending;
    // Virtual first direction (round 3; SCHWZ_CG_P0VIRTUAL=0: stored as before).  A solve that started in the walk
    // has p0 = D^-1 r0 with D^-1 uniform or absent, and r0 is in memory: the first-direction launch then stores
    // nothing (windows and the sums of p0.(A p0) only), the first update walk builds its windows from r0 x D^-1 and
    // writes r1 to the OTHER residual buffer, and r0 -- intact -- serves as p0 for the first fused direction launch
    // and for the x update.  16 n bytes per solve less (the p0 store and one p0 read), the same bits: every reader
    // forms the same rounded product D^-1 r0 the store would have held.
    pl.p0_virtual = env_on("SCHWZ_CG_P0VIRTUAL") && pl.walk_started && all_walks && pl.deferx && !pl.general &&
                    max_iters >= 2;
    // The last iteration of a solve of exactly max_iters iterations (rtol == 0: no stopping test can fire), x
    // deferred: what its result needs is alpha = rho / (p.Ap) and x += alpha p, and both happen inside the last x
    // update.  The residual update r -= alpha A p with rho' and ||r||^2, and the state advance, produce nothing
    // anybody reads -- the next solve starts from b - A y -- unless the caller asks for the iteration count or
    // the residual norm: they are postponed (schwz_pcg::lazy, pcg_finish_lazy) instead of launched.  Same x bit
    // for bit.  SCHWZ_CG_LAZYLAST=0: every iteration is launched in full.
    pl.lazy_last = env_on("SCHWZ_CG_LAZYLAST") && rtol == 0.0 && pl.deferx && !pl.general && max_iters > 0;
    // ... and the direction of that last iteration is never stored (round 3; SCHWZ_CG_PLASTVIRTUAL=0: stored): its
    // only readers are the x update -- which rebuilds it from the direction before it, which it reads anyway, and
    // the current residual: the same fma the fused direction launch performed -- and the postponed update launch,
    // which gets it rebuilt first (cg_rebuild_direction_kernel).  8 n bytes of stores per solve less.
    pl.vlast = pl.lazy_last && env_on("SCHWZ_CG_PLASTVIRTUAL") && max_iters >= 2 && all_walks;
    // Small systems are bound by launches, not bytes (33 k rows: 3 launches of ~3 us work each):
    // kGraphIters iterations are captured once per (x, rtol, plan) into a hipGraph -- on a private stream,
    // the caller's may be the legacy default stream -- and replayed.  SCHWZ_CG_GRAPH=0 disables,
    // =2 uses graphs for every size.
    static const int graph_mode = env_mode("SCHWZ_CG_GRAPH", 1);
    pl.graph = graph_mode != 0 && !pl.general && !g_prof.on && !pl.deferx && (graph_mode == 2 || s->n <= kGraphRows) &&
               max_iters >= kGraphIters;
}

// the bits of schwz_pcg_flavour (include/schwz_hip.h, schwz_pcg::last_flavour)
static int pcg_plan_flavour(const CgPlan &pl, int diag_mode)
{
    return (!pl.qfree ? 0 : (pl.fusedir ? 2 : 1)) | (pl.deferx ? 4 : 0) |
           (pl.sweep_on && pl.deferx && diag_mode != 2 ? 8 : 0) | (pl.sweep_dirdot && pl.fusedir ? 16 : 0) |
           (pl.walk_started ? 32 : 0) | (pl.p0_virtual ? 64 : 0) | (pl.vlast ? 128 : 0);
}

// The buffers the plan needs beyond those of pcg_build, allocated at their first use: the direction ring with
// its alphas (deferred x) and the second residual (virtual first direction).  Without room for them the plan
// falls back: no ring -- false, ring_failed is set and the caller plans again (the plain iteration); no second
// residual -- the stored first direction.
static bool pcg_acquire_buffers(schwz_pcg *s, CgPlan &pl)
{
    const size_t n_pad = (size_t)((s->n + 1) & ~int64_t(1));
    if (pl.deferx && !s->p_ring) {
        s->ring_has_q = pl.qfree;
        if (s->p_ring.alloc(n_pad * (kDeferDepth - (pl.qfree ? 2 : 1))) || s->alpha_hist.alloc(kDeferDepth)) {
            (void)hipGetLastError();
            s->p_ring = Dev<double>();
            s->ring_failed = true;
            return false;
        }
    }
    if (pl.p0_virtual && !s->r_alt && s->r_alt.alloc(n_pad)) {
        (void)hipGetLastError();
        pl.p0_virtual = false;
    }
    return true;
}

// First half of a solve: r = b - A x, p = M^-1 r, rho, ||r||^2 -> CgState.  With
// `fused` the same pass over the matrix also yields ||b - A x2||^2 over the rows
// below row_limit in s->d_norm_sq[0] (x2 == nullptr: x2 is x).
int pcg_begin(schwz_pcg *s, const double *d_b, double *d_x, double rtol, bool fused, const double *d_x2,
              int64_t row_limit, hipStream_t st)
{
    const CsrView &A = s->A->v;
    s->plan = pcg_plan_matrix(s);
    if (!pcg_acquire_buffers(s, s->plan)) s->plan = pcg_plan_matrix(s);
    const CgPlan &pl = s->plan;
    const int gs = pl.gs;
    s->lazy.pending = false;  // nobody asked for the last solve's final residual: it is recomputed from b - A x now
    SpmvArgs a;
    a.x = d_x;
    a.x2 = d_x2;
    a.b = d_b;
    a.y = s->r;
    a.p = s->p;
    a.dinv = s->dinv;
    a.partials = s->partials;
    a.stream_part = s->stream_part;
    a.row_limit = row_limit;
    // x2 == x over all rows: the check residual IS the start residual (rr bank)
    const bool same = fused && d_x2 == nullptr && row_limit >= s->n;
    if (pl.general) a.dinv = nullptr;  // p := r for now, z follows
    if (!pl.general && A.pair_id && s->variant == 0 && s->diag.mode == 3) {
        // row-pair kernel: a uniform Jacobi diagonal travels as a scalar, not as a vector of n equal values
        a.dinv = nullptr;
        a.diag_mode = 3;
        a.diag_uniform = s->diag.uniform;
    }
    // the start launch in the z-sweep walk where the whole solve runs in it (with the second product of the
    // fused check residual only where the upload built its plane flags)
    s->p_pending = pl.sweep_start && (a.diag_mode == 3 || !a.dinv) && (!(fused && !same) || pair_sweep_dual_ok(A, gs));
    s->init = schwz_pcg::InitFold();
    if (s->p_pending) {
        a.sweep_init = 1;
        a.p = nullptr;
        if (pl.initfold) {
            // banks of their own: other workgroups of the launch that folds them may already be writing their partial
            // sums of p0.(A p0) into the SpMV banks while its workgroup 0 still reads these
            a.partials = s->partials + 5 * kMaxGrid;
            s->init.pending = true;
            s->init.partials = a.partials;
            s->init.nparts = gs;
            s->init.rtol = rtol;
            s->init.norm_sq_out = fused ? s->d_norm_sq : nullptr;
            s->init.norm_bank = same ? 1 : 2;
        }
    }
    int rc = launch_spmv(A, (fused && !same) ? kSpmvResidDual : kSpmvResidInit, a, s->variant, st);
    if (rc) return rc;
    if (pl.general) {
        // the check-residual norm (bank 1 or 2 of the SpMV partials) first, then z = M^-1 r,
        // p = z and rho = r.z, ||r||^2 from the vector-kernel partials
        if (fused) {
            if ((rc = launch_final_norm(s->partials + (same ? 1 : 2) * gs, gs, s->d_norm_sq, st))) return rc;
        }
        if ((rc = pcg_apply_general(s, st))) return rc;
        const int gv = grid_for(s->n);
        double *part_vec = s->partials + 3 * kMaxGrid;
        hipLaunchKernelGGL(dot_rz_kernel, dim3(gv), dim3(kBlock), 0, st, s->n, s->r, s->z, s->p, nullptr, 0, part_vec);
        hipLaunchKernelGGL(cg_init_finalize_kernel, dim3(1), dim3(kBlock), 0, st, s->state.dev(), part_vec, gv, rtol, nullptr,
                           1);
        SCHWZ_HIP_TRY(hipGetLastError());
        return SCHWZ_OK;
    }
    if (s->init.pending) return SCHWZ_OK;  // pcg_iterate: the first-direction launch (or, without one, this kernel there)
    hipLaunchKernelGGL(cg_init_finalize_kernel, dim3(1), dim3(kBlock), 0, st, s->state.dev(), s->partials, gs, rtol,
                       fused ? s->d_norm_sq : nullptr, same ? 1 : 2);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

// whether a solve of `s` would defer x as things stand (the ring is acquired on the way, like in pcg_begin): who
// hands the solve an x_out asks first
bool pcg_defers_x(schwz_pcg *s)
{
    CgPlan pl = pcg_plan_matrix(s);
    if (!pcg_acquire_buffers(s, pl)) pl = pcg_plan_matrix(s);
    return pl.deferx;
}

namespace {

// One launch between a pair of HIP events when this is the live solve and bench.py's roofline leg is
// listening (schwz_profile_begin); kind: 0 = a launch that yields p.(A p), 1 = an update launch
template <class Launch>
int profiled(bool live, int kind, hipStream_t q, Launch &&launch)
{
    const bool prof = live && g_prof.on && g_prof.used + 2 <= g_prof.ev.size();
    if (prof) SCHWZ_HIP_TRY(hipEventRecord(g_prof.ev[g_prof.used], q));
    const int rc = launch();
    if (rc) return rc;
    if (prof) {
        SCHWZ_HIP_TRY(hipEventRecord(g_prof.ev[g_prof.used + 1], q));
        g_prof.kind[g_prof.used / 2] = kind;
        g_prof.used += 2;
    }
    return SCHWZ_OK;
}

// The launches of one solve: the plan, what pcg_iterate was given, and one function per step.  `live` marks
// the launches of the solve itself as opposed to those recorded into a graph: only they know which iteration
// is the last one (recorded graphs replay mid-solve) and only they are profiled.
struct CgSolve {
    schwz_pcg *const s;
    const CgPlan pl;
    double *const d_x;
    const double rtol;
    const int max_iters;
    const hipStream_t st;  // the caller's stream
    const CsrView &A;
    const int64_t n;
    const int gs, gv;
    double *const part_spmv;  // [3][gs]
    double *const part_vec;   // [2][gv]
    const int lazy_it;        // the iteration whose update launch is postponed, -1: none
    FlushX fx;
    double *pbuf[2];          // x updated in the launches: p alternates between these with the fused direction launch
    bool prio_recorded = false;
    bool x_moved = false;     // schwz_pcg::x_out: an x update has run, x lives in x_out from here on

    CgSolve(schwz_pcg *s_, const CgPlan &pl_, double *x, double rtol_, int max_iters_, hipStream_t st_)
        : s(s_), pl(pl_), d_x(x), rtol(rtol_), max_iters(max_iters_), st(st_), A(s_->A->v), n(s_->n), gs(pl_.gs),
          gv(pl_.gv), part_spmv(s_->partials), part_vec(s_->partials + 3 * kMaxGrid),
          lazy_it(pl_.lazy_last ? max_iters_ - 1 : -1)
    {
        const int64_t n_pad = (n + 1) & ~int64_t(1);
        for (int k = 0; k < kDeferDepth; ++k)
            fx.ring.slot[k] = k == 0 ? s->p
                                     : (!s->p_ring ? s->p
                                                   : (s->ring_has_q ? (k == 1 ? s->q : s->p_ring + (int64_t)(k - 2) * n_pad)
                                                                    : s->p_ring + (int64_t)(k - 1) * n_pad));
        // virtual first direction: p0 = p0_scale x r0, and slot 0 is r0 where the start launch left it (a later
        // direction 16, 32, ... simply lands there: r0 is done with by then)
        if (pl.p0_virtual) fx.ring.slot[0] = s->r;
        fx.n = n;
        fx.x = s->x_out ? s->x_out : d_x;
        fx.alpha_hist = s->alpha_hist;
        fx.st = s->state.dev();
        fx.fused = pl.qfree ? 0 : 1;  // how the in-launch update of this iteration forms x + alpha p
        fx.pq_partials = part_spmv;   // p.(A p) of the last iteration: SpMV bank 0, gs slots
        fx.pq_nparts = gs;
        fx.x2_src = s->x2_src;
        fx.x2_total = s->x2_total;
        fx.p0_scale = pl.p0_virtual && s->diag.mode != 0 ? s->diag.uniform : 1.0;
        fx.dmode = s->diag.mode;
        fx.dsc = s->diag.uniform;
        pbuf[0] = s->p;
        pbuf[1] = pl.fusedir ? s->q : s->p;
    }

    double *slot(int it) const { return const_cast<double *>(fx.ring.slot[it % kDeferDepth]); }

    // x += sum alpha_k p_k over the iterations [b0, b0 + count) (cg_flush_x_kernel); `last`: this launch finishes x
    void flush_x(int b0, int count, int pending, hipStream_t q, bool last)
    {
        const int64_t n2 = n >> 1;
        // the second output, the alpha of the postponed update and the never-stored last direction only from the
        // launches that finish x
        FlushXLast fl;
        fl.vlast_r = s->r;
        if (last) {
            fl.x2 = s->x2_out;
            fl.x2_rows = s->x2_rows;
            fl.lazy_it = lazy_it;
            fl.vlast_it = pl.vlast ? lazy_it : -1;
        }
        // the first x update of a solve with an x_out reads the caller's vector (and leaves it alone), every later
        // one runs in place on x_out
        const bool oop = s->x_out && !x_moved;
        if (oop) fl.x_in = d_x;
        auto launch = [&](int grid, int64_t pair0, int64_t pair1, int tail) {
            if (oop)
                hipLaunchKernelGGL(cg_flush_x_kernel<true>, dim3(grid), dim3(kBlock), 0, q, fx, fl, b0, count, pending, pair0, pair1, tail);
            else
                hipLaunchKernelGGL(cg_flush_x_kernel<false>, dim3(grid), dim3(kBlock), 0, q, fx, fl, b0, count, pending, pair0, pair1, tail);
        };
        if (last && s->prio_on && s->prio_event && q == st && !prio_recorded) {
            // the caller's priority rows first, the event, then the rest (the same bits: every element is
            // updated by exactly one lane of exactly one of the launches)
            const int64_t lo = std::min(s->prio_lo >> 1, n2), hi = std::max(std::min(s->prio_hi >> 1, n2), lo);
            if (lo > 0) launch(grid_for(lo), 0, lo, 0);
            // (this launch also copies the entries of x2 beyond the solve's vector -- the halo of x~, two planes of a
            // slab --, element by element over its whole grid: sized for that too.  With one workgroup, which is what
            // the upper priority range of a subdomain without an upper neighbour asks for, that copy took 0.44 ms.)
            const int64_t tail_items = fl.x2 ? std::max<int64_t>(s->x2_total - 2 * n2, 0) : 0;
            launch(std::max(grid_for(n2 - hi + 1), grid_for(tail_items)), hi, n2, 1);
            if (hipEventRecord(s->prio_event, q) == hipSuccess) prio_recorded = true;
            if (hi > lo) launch(grid_for(hi - lo), lo, hi, 0);
        } else {
            launch(gv, 0, n2, 1);
        }
        if (fl.x2) s->x2_written = true;
        x_moved = true;
    }

    // the ring is full after iteration `it`: its kDeferDepth increments go into x before slot (it + 1) % depth,
    // the oldest direction, is overwritten
    void flush_full_ring(int it, hipStream_t q, bool last)
    {
        if ((it + 1) % kDeferDepth == 0) flush_x(it + 1 - kDeferDepth, kDeferDepth, it, q, last);
    }

    // p.(A p) on its own launch (every iteration without the fused direction launch)
    int launch_dot(int it, hipStream_t q, bool live)
    {
        SpmvArgs a;
        a.x = pl.deferx ? slot(it) : s->p;
        a.y = s->q;
        a.partials = part_spmv;
        a.stream_part = s->stream_part;
        a.stop_iter = &s->state.dev()->stop_iter;
        a.it = it;
        return profiled(live, 0, q, [&] { return launch_spmv(A, pl.dot_mode, a, s->variant, q); });
    }

    // q = A p is never stored: the update pass recomputes (A p)_i row by row while it streams x and r
    // (spmv_pair.hip, kSpmvCgUpdate): 16 B per row less HBM traffic, a third of the stores of these two launches
    SpmvArgs qfree_update_args(int it, bool first_virtual) const
    {
        SpmvArgs u;
        u.x = pl.deferx ? slot(it) : pbuf[it & 1];
        u.cg_x = pl.deferx ? nullptr : d_x;
        u.alpha_out = pl.deferx ? s->alpha_hist + it % kDeferDepth : nullptr;
        u.cg_r = s->r;
        u.cg_state = s->state.dev();
        u.pq_partials = part_spmv;
        u.pq_nparts = gs;
        u.diag_mode = s->diag.mode;
        u.diag_uniform = s->diag.uniform;
        u.dinv = s->dinv;
        u.partials = part_vec;
        u.it = it;
        u.walk = pl.sweep_on && pl.deferx;
        if (first_virtual) {
            u.ring_scale = fx.p0_scale;  // windows = ring_scale x r0 (u.x: slot 0) = p0
            u.cg_r_out = s->r_alt;
            u.p0_virtual = 1;
        }
        return u;
    }

    // p' = z + beta p into the other buffer and the partial sums of p'.(A p') for the next iteration
    int launch_fused_direction(int it, hipStream_t q, bool live, bool first_virtual)
    {
        SpmvArgs f;
        f.x = pl.deferx ? slot(it) : pbuf[it & 1];
        f.y = pl.deferx ? slot(it + 1) : pbuf[(it + 1) & 1];
        f.cg_r = s->r;
        f.cg_state = s->state.dev();
        f.pq_partials = part_vec;
        f.pq_nparts = gs;
        f.diag_mode = s->diag.mode;
        f.diag_uniform = s->diag.uniform;
        f.dinv = s->dinv;
        f.partials = part_spmv;
        f.it = it;
        f.cg_rtol = rtol;
        f.walk = pl.sweep_dirdot;
        if (first_virtual) {
            f.p_scale = fx.p0_scale;  // p0 = p_scale x r0 (f.x: slot 0)
            f.p0_virtual = 1;
        }
        if (pl.vlast && live && it + 1 == lazy_it) {
            f.y = nullptr;     // windows and sums only: nobody reads this direction from memory
            f.p0_virtual = 1;  // (walk kernels only)
        }
        const int mode = s->diag.mode == 1 ? kSpmvDirDotSymVec : kSpmvDirDotSym;
        return profiled(live, 0, q, [&] { return launch_spmv(A, mode, f, s->variant, q); });
    }

    // r -= alpha q, alpha to the history, x and p untouched: the update of the stored-q iteration with x deferred
    void launch_update_deferred(int it, hipStream_t q) const
    {
        hipLaunchKernelGGL((cg_update_kernel<1, false, true>), dim3(gv), dim3(kBlock), 0, q, n, (double *)nullptr, s->r,
                           (const double *)nullptr, s->q, s->diag, part_spmv, gs, s->state.dev(), it, part_vec,
                           s->alpha_hist + it % kDeferDepth);
    }

    // partial sums per bank the update launch leaves: it ran on the SpMV grid (q-free) or on the vector grid
    int update_parts() const { return pl.qfree ? gs : gv; }

    // The residual update and the state advance of iteration `it`, the last one, wait until somebody asks
    // (schwz_pcg::lazy, pcg_finish_lazy).  The postponed launches outlive this object: they carry a copy of it.
    void postpone_last(int it, hipStream_t q)
    {
        s->lazy_run = [*this, it](hipStream_t qq) -> int {
            if (pl.qfree) {
                // the update launch reads its direction from memory: one that was never stored is rebuilt first
                if (pl.vlast)
                    hipLaunchKernelGGL(cg_rebuild_direction_kernel, dim3(gv), dim3(kBlock), 0, qq, n,
                                       (const double *)slot(it > 0 ? it - 1 : 0), it == 1 ? fx.p0_scale : 1.0,
                                       (const double *)s->r, s->diag.mode, s->diag.uniform, (const CgState *)s->state.dev(), it,
                                       slot(it));
                const int rc = launch_spmv(A, kSpmvCgUpdate, qfree_update_args(it, false), s->variant, qq);
                if (rc) return rc;
            } else {
                launch_update_deferred(it, qq);
            }
            hipLaunchKernelGGL(cg_state_advance_kernel, dim3(1), dim3(kBlock), 0, qq, part_vec, update_parts(), s->state.dev(), it,
                               rtol);
            SCHWZ_HIP_TRY(hipGetLastError());
            return SCHWZ_OK;
        };
        s->lazy.pending = true;
        s->lazy.stream = q;
    }

    // What follows the update launch of an iteration with x deferred: the x update when the ring is full, then the
    // new direction into the next ring slot -- after the last iteration of a solve, where nobody reads it, only
    // the state (cg_state_advance_kernel), and nothing at all when that iteration's update is postponed.
    void close_deferred(int it, hipStream_t q, bool lazy_now, bool last)
    {
        flush_full_ring(it, q, last);
        if (lazy_now)
            postpone_last(it, q);
        else if (last)
            hipLaunchKernelGGL(cg_state_advance_kernel, dim3(1), dim3(kBlock), 0, q, part_vec, update_parts(), s->state.dev(), it,
                               rtol);
        else
            hipLaunchKernelGGL((cg_direction_kernel<1, false>), dim3(gv), dim3(kBlock), 0, q, n, slot(it), s->r, s->diag,
                               part_vec, update_parts(), s->state.dev(), it, rtol, slot(it + 1));
    }

    // q-free iteration (row-pair coded matrices): the update launch, then the fused direction + p.(A p) launch
    // or the direction kernel
    int iterate_qfree(int it, hipStream_t q, bool live)
    {
        const bool first_virtual = pl.p0_virtual && live && it == 0;
        const bool lazy_now = live && it == lazy_it, last = live && it == max_iters - 1;
        const SpmvArgs u = qfree_update_args(it, first_virtual);
        int rc;
        if (!lazy_now && (rc = profiled(live, 1, q, [&] { return launch_spmv(A, kSpmvCgUpdate, u, s->variant, q); })))
            return rc;
        if (first_virtual) std::swap(s->r, s->r_alt);  // r1 (and every later residual) lives in the other buffer
        if (pl.fusedir && !last) {
            // (the last iteration of a solve only needs the direction kernel's state update)
            if (pl.deferx) flush_full_ring(it, q, false);
            return launch_fused_direction(it, q, live, first_virtual);
        }
        if (pl.deferx)
            close_deferred(it, q, lazy_now, last);
        else
            hipLaunchKernelGGL((cg_direction_kernel<1, false>), dim3(gv), dim3(kBlock), 0, q, n, pbuf[it & 1], s->r,
                               s->diag, part_vec, gs, s->state.dev(), it, rtol);
        return SCHWZ_OK;
    }

    // stored q, x deferred: r -= alpha q (24 n bytes instead of 48-56 n), alpha to the history, the new
    // direction into the next ring slot
    int iterate_stored_deferred(int it, hipStream_t q, bool live)
    {
        const bool lazy_now = live && it == lazy_it;
        if (!lazy_now) launch_update_deferred(it, q);
        close_deferred(it, q, lazy_now, live && it == max_iters - 1);
        return SCHWZ_OK;
    }

    // stored q, x updated in the launch.  Scalar Jacobi or no preconditioner: z = D^-1 r inside the vector kernels.
    // General preconditioner: x, r update without one; z = M^-1 r; rho' = r.z; p = z + beta p.
    int iterate_stored(int it, hipStream_t q)
    {
        const DiagView none;
        const DiagView &dg = pl.general ? none : s->diag;
        hipLaunchKernelGGL((cg_update_kernel<1, false>), dim3(gv), dim3(kBlock), 0, q, n, d_x, s->r, s->p, s->q, dg,
                           part_spmv, gs, s->state.dev(), it, part_vec);
        const int gz = pl.general ? grid_for(n) : gv;
        if (pl.general) {
            const int rc = pcg_apply_general(s, q);
            if (rc) return rc;
            hipLaunchKernelGGL(dot_rz_kernel, dim3(gz), dim3(kBlock), 0, q, n, s->r, s->z, (double *)nullptr, s->state.dev(), it,
                               part_vec);
        }
        hipLaunchKernelGGL((cg_direction_kernel<1, false>), dim3(gv), dim3(kBlock), 0, q, n, s->p, pl.general ? s->z : s->r,
                           dg, part_vec, gz, s->state.dev(), it, rtol);
        return SCHWZ_OK;
    }

    // one CG iteration on stream `q`; `it` only enters through its parity (rho slot) and through
    // "it >= stop_iter", and stop_iter is 0 once the tolerance test has fired: a recorded sequence
    // of an even number of iterations can therefore be replayed as a hipGraph
    int iterate(int it, hipStream_t q, bool live)
    {
        int rc;
        if (!pl.fusedir && (rc = launch_dot(it, q, live))) return rc;
        if (pl.qfree) return iterate_qfree(it, q, live);
        return pl.deferx ? iterate_stored_deferred(it, q, live) : iterate_stored(it, q);
    }

    // the recorded run of kGraphIters iterations for this (x, rtol, plan): found, or captured now; *out stays
    // null where capture or instantiation is refused (the solve then launches one by one)
    int graph_for_solve(hipGraphExec_t *out)
    {
        for (const auto &g : s->graphs)
            if (g.x == d_x && g.rtol == rtol && g.variant == s->variant && g.flavour == pl.flavour) *out = g.exec;
        if (*out || s->graphs.size() >= 4) return SCHWZ_OK;
        int rc_cs;
        if (!s->capture_stream && (rc_cs = s->capture_stream.create())) return rc_cs;
        if (hipStreamBeginCapture(s->capture_stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            int rc = SCHWZ_OK;
            for (int k = 0; k < kGraphIters && !rc; ++k) rc = iterate(k, s->capture_stream, false);
            Graph graph;
            const hipError_t e1 = hipStreamEndCapture(s->capture_stream, &graph.h);
            if (rc) return rc;
            if (e1 == hipSuccess && hipGraphInstantiate(out, graph, nullptr, nullptr, 0) == hipSuccess)
                s->graphs.push_back({d_x, rtol, s->variant, pl.flavour, GraphExec(*out)});
            else
                *out = nullptr;
        }
        (void)hipGetLastError();
        return SCHWZ_OK;
    }

    // p0.(A p0): every later p.(A p) comes out of the fused direction launch
    int first_dot()
    {
        SpmvArgs a;
        a.partials = part_spmv;
        a.it = 0;
        if (!pl.walk_started) {
            a.x = s->p;
            a.stop_iter = &s->state.dev()->stop_iter;
            return launch_spmv(A, kSpmvDotSym, a, s->variant, st);
        }
        // z-sweep start: p0 = D^-1 r0 is built here, from the r the launch reads anyway
        a.y = pl.p0_virtual ? nullptr : slot(0);
        a.cg_r = s->r;
        a.cg_state = s->state.dev();
        a.diag_mode = s->diag.mode;
        a.diag_uniform = s->diag.uniform;
        a.sweep_first = 1;
        if (s->init.pending) {
            // ... and its workgroup 0 folds the start launch's partial sums into CgState (and the check norm)
            a.init_fold = 1;
            a.pq_partials = s->init.partials;
            a.pq_nparts = s->init.nparts;
            a.cg_rtol = s->init.rtol;
            a.norm_sq_out = s->init.norm_sq_out;
            a.norm_bank = s->init.norm_bank;
        }
        return launch_spmv(A, kSpmvDirDotSym, a, s->variant, st);
    }
};

}  // namespace

// Second half: up to max_iters CG updates.  With a positive tolerance the host
// looks at the state every `chunk` iterations, one chunk behind the launches, so
// the queue never drains.
int pcg_iterate(schwz_pcg *s, double *d_x, double rtol, int max_iters, hipStream_t st)
{
    CgPlan pl = s->plan;
    pcg_plan_solve(s, pl, rtol, max_iters);
    (void)pcg_acquire_buffers(s, pl);  // (the ring is pcg_begin's; here: the second residual)
    pl.flavour = pcg_plan_flavour(pl, s->diag.mode);
    s->last_flavour = pl.flavour;
    if (pl.walk_started && !(pl.fusedir && pl.sweep_start)) {
        set_error("pcg_iterate: the start launch left p to a first-direction launch this solve does not run");
        return SCHWZ_ERR_INVALID;
    }
    if (s->x_out && !pl.deferx) {
        set_error("pcg_iterate: a result vector of its own (x_out) needs the deferred x update");
        return SCHWZ_ERR_INVALID;
    }
    CgSolve cg(s, pl, d_x, rtol, max_iters, st);
    const bool poll = rtol > 0.0;
    s->x2_written = false;
    int rc;
    hipGraphExec_t replay = nullptr;
    if (pl.graph && (rc = cg.graph_for_solve(&replay))) return rc;
    if (pl.fusedir && max_iters > 0 && (rc = cg.first_dot())) return rc;
    if (s->init.pending && !(pl.fusedir && max_iters > 0 && pl.walk_started)) {
        // no first-direction launch took the fold of the start launch's partial sums along: the kernel of its own
        hipLaunchKernelGGL(cg_init_finalize_kernel, dim3(1), dim3(kBlock), 0, st, s->state.dev(), s->init.partials, s->init.nparts,
                           s->init.rtol, s->init.norm_sq_out, s->init.norm_bank);
        SCHWZ_HIP_TRY(hipGetLastError());
    }
    s->init.pending = false;
    if (s->init_event) {
        // CgState and the check norm are final behind this point of the stream, wherever they were folded
        SCHWZ_HIP_TRY(hipEventRecord(s->init_event, st));
        s->init_event = nullptr;
    }
    s->p_pending = false;
    ChunkSchedule chunks;
    int it = 0;
    bool stopped = false;
    s->state.begin();
    while (it < max_iters && !stopped) {
        const int end = chunks.end(it, max_iters, poll);
        while (it < end) {
            if (replay && it % kGraphIters == 0 && end - it >= kGraphIters) {
                SCHWZ_HIP_TRY(hipGraphLaunch(replay, st));
                it += kGraphIters;
                continue;
            }
            if ((rc = cg.iterate(it, st, true))) return rc;
            ++it;
        }
        SCHWZ_HIP_TRY(hipGetLastError());
        if (poll && it < max_iters) {
            if ((rc = s->state.poll(st, &stopped))) return rc;
            chunks.grow();
        }
    }
    // the increments of the last, partly filled ring (iterations past a tolerance stop are not
    // counted by CgState::iters and add nothing)
    if (pl.deferx && it % kDeferDepth != 0) {
        cg.flush_x(it - it % kDeferDepth, it % kDeferDepth, -1, st, true);
        SCHWZ_HIP_TRY(hipGetLastError());
    }
    // second output asked for, but no launch above was the last x update (ring just emptied, a stop between two
    // rings, no iteration at all): a launch that adds nothing and copies
    // ... likewise for a result vector of its own that no x update has filled yet
    if (pl.deferx && ((s->x2_out && !s->x2_written) || (s->x_out && !cg.x_moved))) {
        cg.flush_x(it, 0, -1, st, true);
        SCHWZ_HIP_TRY(hipGetLastError());
    }
    // priority rows without a split update (x updated inside the iteration, or no iteration at all): final
    // behind the last launch
    if (s->prio_on && s->prio_event && !cg.prio_recorded) SCHWZ_HIP_TRY(hipEventRecord(s->prio_event, st));
    return SCHWZ_OK;
}

}  // namespace schwz

extern "C" {

int schwz_pcg_solve(schwz_pcg *s, const double *d_b, double *d_x, double rtol, int max_iters,
                    int *h_iters, double *h_resnorm, schwz_stream stream)
{
    SCHWZ_REQUIRE(s && d_b && d_x, "schwz_pcg_solve: null argument");
    SCHWZ_REQUIRE(max_iters >= 0, "schwz_pcg_solve: negative max_iters");
    SCHWZ_REQUIRE((reinterpret_cast<uintptr_t>(d_x) & 15) == 0, "schwz_pcg_solve: x must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (s->n == 0) {
        if (h_iters) *h_iters = 0;
        if (h_resnorm) *h_resnorm = 0.0;
        return SCHWZ_OK;
    }
    int rc = pcg_begin(s, d_b, d_x, rtol, false, nullptr, 0, st);
    if (rc) return rc;
    if ((rc = pcg_iterate(s, d_x, rtol, max_iters, st))) return rc;
    if (h_iters || h_resnorm) {
        if ((rc = pcg_finish_lazy(s))) return rc;
        if ((rc = s->state.read(st))) return rc;
        const CgState &h = s->state.host(0);
        if (h_iters) *h_iters = h.iters;
        if (h_resnorm) *h_resnorm = sqrt(h.rr);
        if (h.rr != h.rr) return pcg_take_trs_error(s);
    }
    return SCHWZ_OK;
}

}  // extern "C"
