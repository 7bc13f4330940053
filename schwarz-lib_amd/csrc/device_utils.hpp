// Device-side helpers shared by the kernel translation units (wave64, 256-thread workgroups).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include "schwz_internal.hpp"

namespace schwz {

// ---------------------------------------------------------------------------
// reductions
// ---------------------------------------------------------------------------

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Sum over the 256-thread workgroup; result valid in every thread.
// `red` must hold 4 doubles.  Fixed order => bitwise reproducible.
__device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();  // protect `red` from a previous use
    if (lane == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a
// workgroup-scope release/acquire fence over ALL address spaces, i.e. an
// s_waitcnt vmcnt(0): every global load or store still in flight (the prefetched
// matrix entries of the next tile, the y stores of the previous one) would have
// to land before the barrier.  The tiles only hand LDS data between waves.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// block_sum for N values at once behind ONE pair of barriers, and barriers that order LDS only: global loads and
// stores in flight (the prefetched windows of a walk) stay in flight.  Each value takes block_sum's
// own path -- wave_sum, one slot per wave, (red[0] + red[1]) + (red[2] + red[3]) -- so the bits are block_sum's.
// `red` must hold 4 N doubles.
template <int N>
__device__ __forceinline__ void block_sum_lds(double (&v)[N], double *red)
{
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    lds_barrier();  // protect `red` from a previous use
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[4 * k + w] = v[k];
    }
    lds_barrier();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (red[4 * k] + red[4 * k + 1]) + (red[4 * k + 2] + red[4 * k + 3]);
}

// The lane's part of fold_partials for BANKS banks of `count` partial sums each (bank b at part + b * count): the same
// strided sums in the same order, their loads requested eight per bank at a time instead of one after the other.
template <int BANKS>
__device__ __forceinline__ void fold_lane_sums(const double *part, int count, double (&s)[BANKS])
{
    constexpr int U = 8;
    for (int i0 = threadIdx.x; i0 < count; i0 += U * kBlock) {
        double v[BANKS][U];
#pragma unroll
        for (int b = 0; b < BANKS; ++b)
#pragma unroll
            for (int k = 0; k < U; ++k) v[b][k] = i0 + k * kBlock < count ? part[(size_t)b * count + i0 + k * kBlock] : 0.0;
#pragma unroll
        for (int b = 0; b < BANKS; ++b)
#pragma unroll
            for (int k = 0; k < U; ++k)
                if (i0 + k * kBlock < count) s[b] += v[b][k];
    }
}

// Every workgroup folds the per-workgroup partial sums of the previous launch
// itself (fixed order): no extra launch and no atomics on the critical path.
__device__ __forceinline__ double fold_partials(const double *part, int count, double *red)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += kBlock) s += part[i];
    return block_sum(s, red);
}

// Start of a CG solve: the partial sums its start launch left (banks of nparts slots: rho = r.z, ||r||^2 and, for
// norm_sq_out, bank norm_bank: the check norm) folded into CgState.  One workgroup: cg_init_finalize_kernel, or
// workgroup 0 of the first-direction walk (spmv_pair.hip) -- the same folds in the same order, the same stores.
__device__ __forceinline__ void cg_init_state(CgState *st, const double *partials, int nparts, double rtol,
                                              double *norm_sq_out, int norm_bank, double *red)
{
    const double rho = fold_partials(partials, nparts, red);
    const double rr = fold_partials(partials + nparts, nparts, red);
    if (norm_sq_out) {
        const double n2 = fold_partials(partials + norm_bank * nparts, nparts, red);
        if (threadIdx.x == 0) {
            norm_sq_out[0] = n2;  // may be mapped host memory
            __threadfence_system();
        }
    }
    if (threadIdx.x == 0) {
        st->rho[0] = rho;
        st->rho[1] = 0.0;
        st->rr = rr;
        st->r0 = sqrt(rr);
        st->iters = 0;
        // loop-top test of iteration 0: ||r|| <= rtol*||r_initial||
        st->stop_iter = (sqrt(rr) <= rtol * sqrt(rr)) ? 0 : INT_MAX;
    }
}

// One iteration's advance of CgState by the one lane that holds the folded rho = r.z and ||r||^2 of the new residual
// (cg_direction_kernel, cg_state_advance_kernel and the fused direction launches of spmv_pair.hip).  Other workgroups read
// rho[it & 1] concurrently: the slot written is the other one.  stop_iter = 0, not it + 1: every later launch leaves
// at once whatever iteration index it carries (the recorded launches of a replayed hipGraph carry 0..15 again and
// again); workgroups of THIS launch that read the 0 early skip their part of p, which nobody will read any more.
__device__ __forceinline__ void cg_advance_state(CgState *st, int it, double rho_new, double rr, double rtol)
{
    st->rho[(it + 1) & 1] = rho_new;
    st->rr = rr;
    st->iters = st->iters + 1;
    if (sqrt(rr) <= rtol * st->r0) st->stop_iter = 0;
}

// ---------------------------------------------------------------------------
// streaming vector kernels (cg.hip, bicgstab.hip): 16-byte accesses, the Jacobi diagonal in its DiagView forms
// ---------------------------------------------------------------------------

typedef double vd2 __attribute__((ext_vector_type(2)));

template <bool NT>
__device__ __forceinline__ void store2(double *base, int64_t i, vd2 v)
{
    if (NT)
        __builtin_nontemporal_store(v, reinterpret_cast<vd2 *>(base) + i);
    else
        reinterpret_cast<vd2 *>(base)[i] = v;
}

// 1/diag of rows 2i and 2i+1 in whichever representation the solver holds
__device__ __forceinline__ vd2 diag_pair(const DiagView &dg, const vd2 *full2, const uint16_t *code2,
                                         const double *ddict, int64_t i)
{
    vd2 d;
    if (dg.mode == 1) {
        d = full2[i];
    } else if (dg.mode == 2) {
        const unsigned c = code2[i];
        d.x = ddict[c & 255u];
        d.y = ddict[c >> 8];
    } else {
        d.x = d.y = dg.uniform;
    }
    return d;
}

__device__ __forceinline__ double diag_one(const DiagView &dg, const double *ddict, int64_t i)
{
    if (dg.mode == 1) return dg.full[i];
    if (dg.mode == 2) return ddict[dg.code[i]];
    return dg.uniform;
}

// Tile dealt to XCD `xcd` as its j-th one.  Tiles go to the eight XCDs (blockIdx % 8) in runs
// of A.xcd_block (block-cyclic; a run as long as an eighth of the matrix gives each XCD one
// contiguous eighth).  The run length was meant to keep the x lines a tile shares with its
// +-nx*ny neighbours inside one XCD's L2; measured on the 256^3 Poisson matrix it changes neither
// the time nor (by more than 4 %) the fetched bytes -- at ~0.5 MB/us of matrix stream per XCD an
// L2 line lives ~9 us, too short for reuse across tiles -- so it only serves load balance.
// Returns -1 past the end.
__device__ __forceinline__ int xcd_tile(const CsrView &A, int xcd, int j)
{
    const int sh = A.xcd_shift;  // xcd_block = 1 << sh
    const int tile = ((j >> sh) << (sh + 3)) + (xcd << sh) + (j & (A.xcd_block - 1));
    return tile < A.ntiles ? tile : -1;
}

}  // namespace schwz
