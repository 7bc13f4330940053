// The straight-line tile pipeline over plain CSR, once: spmv_stream_kernel (spmv_stream.hip), cheb_stream_kernel
// (chebyshev.hip) and f32_spmv_stream_kernel (cg_f32.hip) are a prologue, SCHWZ_STREAM_PIPELINE and an epilogue.
//
// A workgroup goes through tiles of at most kTileRows rows and kTileNnz entries (CsrView::tile_row / tile_nz), and
// nothing in its tile loop waits for a chain of dependent loads:
//   * the tile bounds come from two tables indexed by the tile number alone (tile_row, tile_nz = rp[tile_row]),
//     read two tiles ahead with scalar loads;
//   * the val / col quads, the lane's row start and the own-row operands of the epilogue of tile k + 2 are requested
//     as soon as the products of tile k are in LDS, into the register set tile k has just released (two sets, loop
//     unrolled by two: no register copies), and fly during the barrier, the row sums, the store and the next tile's
//     gathers;
//   * there is no branch in the loop: addresses are clamped instead of guarded (lanes past the tile's last row
//     repeat its last row), the row sum is CAP masked adds in CSR order (an absent entry adds +0.0, which leaves a
//     sum that began at +0.0 unchanged bit for bit).  What a lane past the last row does with its repeated row is
//     the kernel's business: `mine` tells its row epilogue.
// The deal: tiles go to the eight XCDs block-cyclically (or by the explicit CsrView::stream_order of wide planes).
// seq > 0: a workgroup takes `seq` CONSECUTIVE slots of its XCD's sequence and ends, the grid covers the matrix once
// and the dispatch order keeps the active rows a compact moving window (profiles/r03_stream_seq.txt); seq == 0:
// persistent workgroups striding through the sequence.
//
// The form: macros, not a function template.  As a __forceinline__ template over a policy type (register sets as
// structs, issue and step as always-inline lambdas) the pipeline kept its registers out of scratch memory, but hipcc
// then requests all the gathers of the second step of a pair up front at CAP = 32: 212-230 registers instead of
// 142-163 and two waves per SIMD instead of three (profiles/r18_stream_pipeline.txt).  The text below compiles to
// what the three kernels compiled to when each had its own copy; tests/test_stream_pipeline_resources.py holds every
// instantiation to that.
//
// SCHWZ_STREAM_PIPELINE(CSR, CAP, T, VAL, G, SEQ, PERSIST, OPS, LOAD, ROW) in a kernel of kBlock lanes:
//   CSR    the CsrView
//   T      double or float: matrix values, gathered vector, row sum
//   VAL    const T *: the matrix values, entry for entry beside CSR.col
//   G      const T *: the gathered vector
//   SEQ    see above
//   PERSIST  a constant: false where SEQ == 0 never occurs (the Chebyshev launches), which takes the persistent deal,
//          its division and its branches out of the kernel -- 1 % of a 46 us launch (profiles/r18_stream_pipeline.txt)
//   OPS    a struct: the own-row operands of the row epilogue, loaded with the tile's stream
//   LOAD   OPS LOAD(int rowc)
//   ROW    void ROW(T sum, const OPS &o, int rowc, bool mine): the row epilogue; the accumulators are the kernel's
#pragma once

#include <hip/hip_runtime.h>

#include "schwz_internal.hpp"
#include "device_utils.hpp"

namespace schwz {

typedef int vi4 __attribute__((ext_vector_type(4)));
typedef float vf4 __attribute__((ext_vector_type(4)));

struct TileMeta {
    int r0, r1, s, e;  // rows [r0, r1), entries [s, e)
};

// four consecutive matrix values in registers: two 16-byte loads of fp64, one of fp32
template <typename T>
struct ValueQuad;

template <>
struct ValueQuad<double> {
    vd2 lo, hi;
    __device__ __forceinline__ void load(const double *p)
    {
        lo = *reinterpret_cast<const vd2 *>(p);
        hi = *reinterpret_cast<const vd2 *>(p + 2);
    }
    __device__ __forceinline__ void store(double *p) const
    {
        *reinterpret_cast<vd2 *>(p) = lo;
        *reinterpret_cast<vd2 *>(p + 2) = hi;
    }
};

template <>
struct ValueQuad<float> {
    vf4 v;
    __device__ __forceinline__ void load(const float *p) { v = *reinterpret_cast<const vf4 *>(p); }
    __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<vf4 *>(p) = v; }
};

}  // namespace schwz

// Requests the stream of tile M into register set P (S0 or S1): the two quads of values and columns of the lane, its
// row start and its own-row operands.  Every address is clamped into the tile, so nothing is guarded.
#define SCHWZ_TILE_ISSUE(CSR, M, P, VAL, LOAD)                                                                       \
    {                                                                                                                \
        const int s2_ = (M).s & ~3;                                                                                  \
        const int last_ = max(((M).e - 1) & ~3, s2_);                                                                \
        const int i0_ = min(s2_ + 4 * tid_, last_), i1_ = min(s2_ + 4 * (tid_ + kBlock), last_);                     \
        P##v0.load((VAL) + i0_);                                                                                     \
        P##c0 = *reinterpret_cast<const vi4 *>((CSR).col + i0_);                                                     \
        P##v1.load((VAL) + i1_);                                                                                     \
        P##c1 = *reinterpret_cast<const vi4 *>((CSR).col + i1_);                                                     \
        const int rowc_ = min((M).r0 + tid_, (M).r1 - 1);                                                            \
        /* ONE row-pointer load per lane: the end of a row is the start of the next lane's, handed */                \
        /* over through LDS in the step; the tile's last row ends where the tile does (M.e) */                       \
        P##b0 = (CSR).rp[rowc_] - s2_;                                                                               \
        P##o = LOAD(rowc_);                                                                                          \
    }

// One tile: set P holds its stream on entry and the stream of tile MN (two tiles on) on exit.  The entries go to LDS
// as they are stored; then a lane IS a row: entry j of 64 consecutive rows per gather instruction (for a stencil: one
// contiguous run of the vector), products rounded one by one and added in CSR order.  The next stream is requested
// AFTER the first eight gathers (the scheduling barriers keep hipcc from moving it up), so that waiting for them --
// an in-order counter -- does not wait for it.  The last two steps of a workgroup request its last tile again: no
// branch.  The barriers order LDS traffic only (lds_barrier): the loads in flight stay in flight.
// (Keeping the gathered operands of a tile for a step and summing one step later -- a whole step of slack for the
// gathers, 126-157 registers -- measured the same: the launch is not bound by the latency of its gathers.)
#define SCHWZ_TILE_STEP(CSR, M, MN, P, CAP, T, VAL, G, LOAD, ROW)                                                    \
    {                                                                                                                \
        const int b0 = P##b0;                                                                                        \
        const auto o_ = P##o;                                                                                        \
        lds_barrier(); /* every lane is done with the previous tile's entries */                                     \
        rstart_[tid_] = b0;                                                                                          \
        P##v0.store(&vals_[4 * tid_]);                                                                               \
        *reinterpret_cast<vi4 *>(&cols_[4 * tid_]) = P##c0;                                                          \
        P##v1.store(&vals_[4 * (tid_ + kBlock)]);                                                                    \
        *reinterpret_cast<vi4 *>(&cols_[4 * (tid_ + kBlock)]) = P##c1;                                               \
        lds_barrier();                                                                                               \
        const int b1 = (M).r0 + tid_ + 1 < (M).r1 ? rstart_[tid_ + 1] : (M).e - ((M).s & ~3);                        \
        T sum = T(0);                                                                                                \
        _Pragma("unroll") for (int j0 = 0; j0 < CAP; j0 += 8)                                                        \
        {                                                                                                            \
            T vv[8], xx[8];                                                                                          \
            int cc[8];                                                                                               \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                            \
            {                                                                                                        \
                vv[j] = vals_[b0 + j0 + j];                                                                          \
                cc[j] = cols_[b0 + j0 + j];                                                                          \
            }                                                                                                        \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) xx[j] = (G)[cc[j]];                                        \
            if (j0 == 0) {                                                                                           \
                __builtin_amdgcn_sched_barrier(0);                                                                   \
                SCHWZ_TILE_ISSUE(CSR, MN, P, VAL, LOAD)                                                              \
                __builtin_amdgcn_sched_barrier(0);                                                                   \
            }                                                                                                        \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                            \
            {                                                                                                        \
                const T pv = vv[j] * xx[j];                                                                          \
                sum += (b0 + j0 + j < b1) ? pv : T(0);                                                               \
            }                                                                                                        \
        }                                                                                                            \
        ROW(sum, o_, min((M).r0 + tid_, (M).r1 - 1), (M).r0 + tid_ < (M).r1);                                        \
    }

// The LDS arrays with their finite tail, the deal, the tile tables and the driver over the two register sets.
#define SCHWZ_STREAM_PIPELINE(CSR, CAP, T, VAL, G, SEQ, PERSIST, OPS, LOAD, ROW)                                     \
    {                                                                                                                \
        /* the tile's values and columns as stored (16-byte aligned window of <= kTileNnz entries, */                \
        /* + what the masked reads of the last rows may touch) */                                                    \
        __shared__ __attribute__((aligned(16))) T vals_[kTileNnz + 4 + CAP];                                         \
        __shared__ __attribute__((aligned(16))) int cols_[kTileNnz + 4 + CAP];                                       \
        __shared__ int rstart_[kBlock + 1]; /* first entry of every row of the tile (window-relative) */             \
        const int tid_ = threadIdx.x;                                                                                \
        const int xcd_ = blockIdx.x % kXcds;                                                                         \
        const int slot_ = blockIdx.x / kXcds;                                                                        \
        const int per_xcd_ = gridDim.x / kXcds;                                                                      \
        /* an XCD's tile sequence: block-cyclic, or the explicit one of wide planes (entries past the end */         \
        /* are -1, mapped to ntiles = "no tile" here); read through the scalar cache */                              \
        typedef const int __attribute__((address_space(4))) *const_ints_;                                            \
        const const_ints_ sorder_ = (const_ints_)(uintptr_t)(CSR).stream_order;                                      \
        const int nslots_ = stream_slots(CSR);                                                                       \
        const int sh_ = (CSR).xcd_shift;                                                                             \
        auto tile_at_ = [&](int j) -> int {                                                                          \
            if (sorder_) {                                                                                           \
                const int t = sorder_[(int64_t)xcd_ * (CSR).stream_nper + j];                                        \
                return t < 0 ? (CSR).ntiles : t;                                                                     \
            }                                                                                                        \
            return ((j >> sh_) << (sh_ + 3)) + (xcd_ << sh_) + (j & ((CSR).xcd_block - 1));                          \
        };                                                                                                           \
        /* tiles of this workgroup: k = 0 .. ntw_ - 1 (past-the-end slots only occur at the tail of the deal) */     \
        const int seq_ = (SEQ);                                                                                      \
        auto slot_at_ = [&](int k) -> int {                                                                          \
            return (!(PERSIST) || seq_) ? slot_ * seq_ + k : slot_ + k * per_xcd_;                                   \
        };                                                                                                           \
        int ntw_ = (!(PERSIST) || seq_) ? max(0, min(seq_, nslots_ - slot_ * seq_))                                  \
                                        : (slot_ < nslots_ ? (nslots_ - slot_ + per_xcd_ - 1) / per_xcd_ : 0);       \
        while (ntw_ > 0 && tile_at_(slot_at_(ntw_ - 1)) >= (CSR).ntiles) --ntw_;                                     \
        /* the masked reads of a tile's last rows may run up to CAP entries past the window: keep that */            \
        /* tail finite and inside the gathered vector (it is never summed, but its columns are gathered) */          \
        if (tid_ < 4 + CAP) {                                                                                        \
            vals_[kTileNnz + tid_] = T(0);                                                                           \
            cols_[kTileNnz + tid_] = 0;                                                                              \
        }                                                                                                            \
        if (ntw_ > 0) {                                                                                              \
            const const_ints_ trow_ = (const_ints_)(uintptr_t)(CSR).tile_row;                                        \
            const const_ints_ tnz_ = (const_ints_)(uintptr_t)(CSR).tile_nz;                                          \
            auto meta_ = [&](int k) -> TileMeta {                                                                    \
                /* beyond the workgroup's last tile: loaded (no branch in the loop), never computed -- one */        \
                /* quad and one row of the last tile, so that every such load touches a single line */               \
                const int t = tile_at_(slot_at_(min(k, ntw_ - 1)));                                                  \
                const bool past = k >= ntw_;                                                                         \
                const int r0 = trow_[t], s0 = tnz_[t];                                                               \
                return TileMeta{r0, past ? r0 + 1 : trow_[t + 1], s0, past ? s0 : tnz_[t + 1]};                      \
            };                                                                                                       \
            /* two register sets: tiles k and k + 1 in flight / landed */                                            \
            ValueQuad<T> S0v0, S0v1, S1v0, S1v1;                                                                     \
            vi4 S0c0, S0c1, S1c0, S1c1;                                                                              \
            int S0b0, S1b0;                                                                                          \
            OPS S0o, S1o;                                                                                            \
            TileMeta m0 = meta_(0), m1 = meta_(1);                                                                   \
            SCHWZ_TILE_ISSUE(CSR, m0, S0, VAL, LOAD)                                                                 \
            SCHWZ_TILE_ISSUE(CSR, m1, S1, VAL, LOAD)                                                                 \
            TileMeta m2 = meta_(2), m3 = meta_(3);                                                                   \
            int k = 0;                                                                                               \
            for (; k + 1 < ntw_; k += 2) {                                                                           \
                SCHWZ_TILE_STEP(CSR, m0, m2, S0, CAP, T, VAL, G, LOAD, ROW)                                          \
                SCHWZ_TILE_STEP(CSR, m1, m3, S1, CAP, T, VAL, G, LOAD, ROW)                                          \
                m0 = m2;                                                                                             \
                m1 = m3;                                                                                             \
                m2 = meta_(k + 4);                                                                                   \
                m3 = meta_(k + 5);                                                                                   \
            }                                                                                                        \
            if (k < ntw_) SCHWZ_TILE_STEP(CSR, m0, m2, S0, CAP, T, VAL, G, LOAD, ROW)                                \
        }                                                                                                            \
    }
