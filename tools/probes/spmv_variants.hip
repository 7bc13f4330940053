// SpMV experiments that were measured and NOT kept: one row per lane, the first tiled
// kernel, software-pipelined tiles, wave-private tiles and the ablation builds of the tiled kernel -- variant ids
// 1-5 and 10-73 of schwz_csr_spmv -- plus the macro form of the stream kernel with its ablation builds (80 + bits).
// Linked into the measurement build libschwz_hip_probes.so only (`make -C schwarz-lib_amd probes`), which
// tools/spmv_probe.py, tools/stream_ablate.py and tools/r03_stream_probe.py load through SCHWZ_HIP_LIB; the
// product library holds none of this.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "schwz_internal.hpp"
#include "device_utils.hpp"

namespace schwz {

constexpr int kPairsPerLane = kTileNnz / (2 * kBlock);  // 16-byte (value, column) pairs per lane and tile: 4

// ---------------------------------------------------------------------------
// CSR SpMV, tiled: each workgroup owns a run of consecutive rows whose nonzeros
// (<= kTileNnz) are read with unit stride, multiplied with the gathered x and
// staged in LDS; one lane per row then sums its LDS segment.  Tiles are dealt to
// workgroups so that each XCD (blockIdx % 8) sweeps one contiguous eighth of the
// matrix: the x entries a tile shares with its neighbours (i+-1, i+-nx, i+-nx*ny
// for the Poisson stencils) stay in that XCD's 4 MiB L2.
// ---------------------------------------------------------------------------

template <int MODE>
__global__ __launch_bounds__(kBlock) void spmv_tiled_kernel(CsrView A, SpmvArgs a)
{
    // every SpMV variant rounds each product before it is added (no FMA contraction), so
    // that all variants -- and the sequential CPU oracle -- produce the same bits
#pragma clang fp contract(off)
    __shared__ double prod[kTileNnz];
    __shared__ double red[4];
    if (MODE == kSpmvDot || MODE == kSpmvResidInit) {
        if (a.stop_iter && a.it >= *a.stop_iter) return;
    }
    const int tid = threadIdx.x;
    const int xcd = blockIdx.x % kXcds;
    const int slot = blockIdx.x / kXcds;
    const int per_xcd = gridDim.x / kXcds;
    const int chunk = (A.ntiles + kXcds - 1) / kXcds;
    double acc0 = 0.0, acc1 = 0.0;

    for (int t = slot; t < chunk; t += per_xcd) {
        const int tile = xcd * chunk + t;
        if (tile >= A.ntiles) break;
        const int r0 = A.tile_row[tile], r1 = A.tile_row[tile + 1];
        const int s = A.rp[r0], e = A.rp[r1];
        const int cnt = e - s;
        double sum = 0.0;
        int row = r0 + tid;
        bool have_row = false;
        if (cnt <= kTileNnz) {
            for (int i = tid; i < cnt; i += kBlock)
                prod[i] = A.val[s + i] * a.x[A.col[s + i]];
            __syncthreads();
            if (row < r1) {
                have_row = true;
                const int b0 = A.rp[row] - s, b1 = A.rp[row + 1] - s;
                for (int j = b0; j < b1; ++j) sum += prod[j];
            }
            __syncthreads();
        } else {
            // a single row longer than a tile: the whole workgroup reduces it
            double part = 0.0;
            for (int i = tid; i < cnt; i += kBlock) part += __dmul_rn(A.val[s + i], a.x[A.col[s + i]]);
            part = block_sum(part, red);
            row = r0;
            if (tid == 0) {
                have_row = true;
                sum = part;
            }
        }
        if (have_row) {
            if (MODE == kSpmvPlain) {
                a.y[row] = (a.beta == 0.0) ? a.alpha * sum : a.alpha * sum + a.beta * a.y[row];
            } else if (MODE == kSpmvDot) {
                a.y[row] = sum;
                acc0 += a.x[row] * sum;
            } else if (MODE == kSpmvResidInit) {
                const double r = a.b[row] - sum;
                const double z = a.dinv ? a.dinv[row] * r : r;
                a.y[row] = r;
                a.p[row] = z;
                acc0 += r * z;
                acc1 += r * r;
            } else {  // kSpmvResidNorm
                if (row < a.row_limit) {
                    const double r = a.b[row] - sum;
                    acc1 += r * r;
                }
            }
        }
    }
    if (MODE != kSpmvPlain) {
        const double s0 = block_sum(acc0, red);
        const double s1 = block_sum(acc1, red);
        if (tid == 0) {
            a.partials[blockIdx.x] = s0;
            a.partials[gridDim.x + blockIdx.x] = s1;
        }
    }
}


// ---------------------------------------------------------------------------
// Software-pipelined tiled SpMV (variant 4; measured no faster than variant 0).  Same tiles and arithmetic
// as spmv_tiled2_kernel, but a workgroup's tile loop is a two-stage pipeline:
// as soon as the products of tile t are in LDS, the 16-byte loads of tile t+1 are
// issued into the SAME registers, so they fly during the barrier / row-sum / store
// phase of tile t; the tile descriptors (row range, nonzero range) are fetched one
// tile ahead as well.  Each workgroup thus always has ~24 KiB of matrix stream in
// flight instead of stalling through a load -> gather -> LDS -> barrier chain.
// ---------------------------------------------------------------------------

struct TileDesc {
    int r0, r1, s, e;
    bool valid, regular;
};

__device__ __forceinline__ TileDesc tile_desc(const CsrView &A, int xcd, int chunk, int t)
{
    TileDesc d;
    d.r0 = d.r1 = d.s = d.e = 0;
    d.regular = false;
    const int tile = t < chunk ? xcd_tile(A, xcd, t) : -1;
    d.valid = tile >= 0;
    if (d.valid) {
        const int tl = A.tile_order ? A.tile_order[tile] : tile;
        d.r0 = A.tile_row[tl];
        d.r1 = A.tile_row[tl + 1];
        d.s = A.rp[d.r0];
        d.e = A.rp[d.r1];
        d.regular = (d.e - d.s) <= kTileNnz - 2;
    }
    return d;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void spmv_pipe_kernel(CsrView A, SpmvArgs a)
{
    // every SpMV variant rounds each product before it is added (no FMA contraction), so
    // that all variants -- and the sequential CPU oracle -- produce the same bits
#pragma clang fp contract(off)
    __shared__ double prod[kTileNnz + 2];
    __shared__ double red[4];
    if (MODE == kSpmvDot || MODE == kSpmvResidInit) {
        if (a.stop_iter && a.it >= *a.stop_iter) return;
    }
    const int tid = threadIdx.x;
    const int xcd = blockIdx.x % kXcds;
    const int slot = blockIdx.x / kXcds;
    const int per_xcd = gridDim.x / kXcds;
    const int chunk = xcd_slots(A);
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    const bool dual = (MODE == kSpmvResidDual) && a.x2 != nullptr;

    double2 v[kPairsPerLane];
    int2 c[kPairsPerLane];
    // No per-pair bounds branch: a lane whose pair lies past the tile re-reads the
    // tile's last pair instead (its product lands in an LDS slot no row sums), so
    // all loads of a phase issue back to back and one wait covers them.
#define SCHWZ_ISSUE_LOADS(D)                                                     \
    {                                                                            \
        const int s2_ = (D).s & ~1;                                              \
        const int last_ = max(((D).e - 1) & ~1, s2_);                            \
        _Pragma("unroll") for (int k = 0; k < kPairsPerLane; ++k)                \
        {                                                                        \
            const int idx = min(s2_ + 2 * (tid + kBlock * k), last_);            \
            v[k] = *reinterpret_cast<const double2 *>(A.val + idx);              \
            c[k] = *reinterpret_cast<const int2 *>(A.col + idx);                 \
        }                                                                        \
    }
#define SCHWZ_PRODUCTS(XV, D)                                                    \
    {                                                                            \
        double xg[2 * kPairsPerLane];                                            \
        _Pragma("unroll") for (int k = 0; k < kPairsPerLane; ++k)                \
        {                                                                        \
            xg[2 * k] = (XV)[c[k].x];                                            \
            xg[2 * k + 1] = (XV)[c[k].y];                                        \
        }                                                                        \
        _Pragma("unroll") for (int k = 0; k < kPairsPerLane; ++k)                \
        {                                                                        \
            double2 pr;                                                          \
            pr.x = v[k].x * xg[2 * k];                                           \
            pr.y = v[k].y * xg[2 * k + 1];                                       \
            *reinterpret_cast<double2 *>(&prod[2 * (tid + kBlock * k)]) = pr;    \
        }                                                                        \
    }

    // past-the-end slots only occur in the last run of the block-cyclic deal
    int t = slot;
    while (t < chunk && xcd_tile(A, xcd, t) < 0) t += per_xcd;
    TileDesc cur = tile_desc(A, xcd, chunk, t);
    if (cur.valid && cur.regular) SCHWZ_ISSUE_LOADS(cur)
    while (cur.valid) {
        t += per_xcd;
        while (t < chunk && xcd_tile(A, xcd, t) < 0) t += per_xcd;
        const TileDesc nxt = tile_desc(A, xcd, chunk, t);
        const int r0 = cur.r0, r1 = cur.r1, s = cur.s, e = cur.e;
        const int cnt = e - s;
        double sum = 0.0, sum2 = 0.0;
        int row = r0 + tid;
        bool have_row = false;
        if (cur.regular) {
            const int s2 = s & ~1;
            int b0 = 0, b1 = 0;
            if (row < r1) {
                b0 = A.rp[row] - s2;
                b1 = A.rp[row + 1] - s2;
            }
            SCHWZ_PRODUCTS(a.x, cur)
            if (!dual && nxt.valid && nxt.regular) SCHWZ_ISSUE_LOADS(nxt)
            lds_barrier();
            if (row < r1) {
                have_row = true;
                for (int j = b0; j < b1; ++j) sum += prod[j];
            }
            lds_barrier();
            if (dual) {
                SCHWZ_PRODUCTS(a.x2, cur)
                if (nxt.valid && nxt.regular) SCHWZ_ISSUE_LOADS(nxt)
                lds_barrier();
                if (row < r1)
                    for (int j = b0; j < b1; ++j) sum2 += prod[j];
                lds_barrier();
            }
        } else {
            if (r1 - r0 > 1) {
                // fits kTileNnz but not the aligned window: plain staging
                for (int i = tid; i < cnt; i += kBlock) prod[i] = A.val[s + i] * a.x[A.col[s + i]];
                lds_barrier();
                const int b0 = row < r1 ? A.rp[row] - s : 0, b1 = row < r1 ? A.rp[row + 1] - s : 0;
                if (row < r1) {
                    have_row = true;
                    for (int j = b0; j < b1; ++j) sum += prod[j];
                }
                lds_barrier();
                if (dual) {
                    for (int i = tid; i < cnt; i += kBlock) prod[i] = A.val[s + i] * a.x2[A.col[s + i]];
                    lds_barrier();
                    for (int j = b0; j < b1; ++j) sum2 += prod[j];
                    lds_barrier();
                }
            } else {
                // a single long row: the whole workgroup reduces it
                double part = 0.0, part2 = 0.0;
                for (int i = tid; i < cnt; i += kBlock) {
                    part += __dmul_rn(A.val[s + i], a.x[A.col[s + i]]);
                    if (dual) part2 += __dmul_rn(A.val[s + i], a.x2[A.col[s + i]]);
                }
                part = block_sum(part, red);
                if (dual) part2 = block_sum(part2, red);
                row = r0;
                if (tid == 0) {
                    have_row = true;
                    sum = part;
                    sum2 = part2;
                }
            }
            if (nxt.valid && nxt.regular) SCHWZ_ISSUE_LOADS(nxt)
        }
        if (have_row) {
            if (MODE == kSpmvPlain) {
                a.y[row] = (a.beta == 0.0) ? a.alpha * sum : a.alpha * sum + a.beta * a.y[row];
            } else if (MODE == kSpmvDot) {
                a.y[row] = sum;
                acc0 += a.x[row] * sum;
            } else if (MODE == kSpmvResidInit || MODE == kSpmvResidDual) {
                const double bb = a.b[row];
                const double r = bb - sum;
                const double z = a.dinv ? a.dinv[row] * r : r;
                a.y[row] = r;
                a.p[row] = z;
                acc0 += r * z;
                acc1 += r * r;
                if (MODE == kSpmvResidDual && row < a.row_limit) {
                    const double r2 = dual ? bb - sum2 : r;
                    acc2 += r2 * r2;
                }
            } else {  // kSpmvResidNorm
                if (row < a.row_limit) {
                    const double r = a.b[row] - sum;
                    acc1 += r * r;
                }
            }
        }
        cur = nxt;
    }
#undef SCHWZ_ISSUE_LOADS
#undef SCHWZ_PRODUCTS
    if (MODE != kSpmvPlain) {
        const double s0 = block_sum(acc0, red);
        const double s1 = block_sum(acc1, red);
        if (tid == 0) {
            a.partials[blockIdx.x] = s0;
            a.partials[gridDim.x + blockIdx.x] = s1;
        }
        if (MODE == kSpmvResidDual) {
            const double s2v = block_sum(acc2, red);
            if (tid == 0) a.partials[2 * gridDim.x + blockIdx.x] = s2v;
        }
    }
}

// ---------------------------------------------------------------------------
// Ablation build of the tiled kernel (plain mode only, WRONG results on purpose):
// used by tools/spmv_probe.py --variants 10.. to price the pieces of a tile.
//   bit 0: no x gather (x := 1)      bit 1: no LDS staging / barriers / row sums
//   bit 2: no y store                bit 3: no column-index stream
// ---------------------------------------------------------------------------
template <int WHAT>
__global__ __launch_bounds__(kBlock) void spmv_ablate_kernel(CsrView A, SpmvArgs a)
{
    __shared__ double prod[kTileNnz + 2];
    const int tid = threadIdx.x;
    const int xcd = blockIdx.x % kXcds;
    const int slot = blockIdx.x / kXcds;
    const int per_xcd = gridDim.x / kXcds;
    const int chunk = xcd_slots(A);
    double keep = 0.0;
    for (int t = slot; t < chunk; t += per_xcd) {
        const int tile = xcd_tile(A, xcd, t);
        if (tile < 0) continue;
        const int r0 = A.tile_row[tile], r1 = A.tile_row[tile + 1];
        const int s = A.rp[r0], e = A.rp[r1];
        if (e - s > kTileNnz - 2) continue;
        const int row = r0 + tid;
        const int s2 = (WHAT & 32) ? s : (s & ~1);
        int b0 = 0, b1 = 0;
        if (row < r1) {
            b0 = A.rp[row] - s2;
            b1 = A.rp[row + 1] - s2;
        }
        double sum = 0.0;
        if (WHAT & 32) {
            // consecutive lanes take consecutive entries (8-byte / 4-byte loads)
            const int last = max(e - 1, s);
            double v[2 * kPairsPerLane];
            int c[2 * kPairsPerLane];
#pragma unroll
            for (int k = 0; k < 2 * kPairsPerLane; ++k) {
                const int idx = min(s + tid + kBlock * k, last);
                v[k] = A.val[idx];
                c[k] = A.col[idx];
            }
            double xg[2 * kPairsPerLane];
#pragma unroll
            for (int k = 0; k < 2 * kPairsPerLane; ++k) xg[k] = a.x[c[k]];
#pragma unroll
            for (int k = 0; k < 2 * kPairsPerLane; ++k) prod[tid + kBlock * k] = v[k] * xg[k];
            lds_barrier();
            if (row < r1)
                for (int j = b0; j < b1; ++j) sum += prod[j];
            lds_barrier();
        } else {
            const int last = max((e - 1) & ~1, s2);
            double2 v[kPairsPerLane];
            int2 c[kPairsPerLane];
#pragma unroll
            for (int k = 0; k < kPairsPerLane; ++k) {
                const int idx = min(s2 + 2 * (tid + kBlock * k), last);
                v[k] = *reinterpret_cast<const double2 *>(A.val + idx);
                if (WHAT & 8) {
                    c[k].x = idx & 1023;
                    c[k].y = (idx + 1) & 1023;
                } else {
                    c[k] = *reinterpret_cast<const int2 *>(A.col + idx);
                }
            }
            double xg[2 * kPairsPerLane];
#pragma unroll
            for (int k = 0; k < kPairsPerLane; ++k) {
                if (WHAT & 1) {
                    xg[2 * k] = 1.0 + c[k].x;
                    xg[2 * k + 1] = 1.0 + c[k].y;
                } else {
                    xg[2 * k] = a.x[c[k].x];
                    xg[2 * k + 1] = a.x[c[k].y];
                }
            }
            if (WHAT & 2) {
#pragma unroll
                for (int k = 0; k < kPairsPerLane; ++k) sum += v[k].x * xg[2 * k] + v[k].y * xg[2 * k + 1];
                sum += b0 + b1;
            } else {
#pragma unroll
                for (int k = 0; k < kPairsPerLane; ++k) {
                    double2 pr;
                    pr.x = v[k].x * xg[2 * k];
                    pr.y = v[k].y * xg[2 * k + 1];
                    *reinterpret_cast<double2 *>(&prod[2 * (tid + kBlock * k)]) = pr;
                }
                lds_barrier();
                if (row < r1)
                    for (int j = b0; j < b1; ++j) sum += prod[j];
                lds_barrier();
            }
        }
        if (WHAT & 4) {
            keep += sum;
        } else if (WHAT & 16) {
            if (row < r1) __builtin_nontemporal_store(sum, &a.y[row]);
        } else if (row < r1) {
            a.y[row] = sum;
        }
    }
    if ((WHAT & 4) && keep == 123.456) a.y[0] = keep;
}

// ---------------------------------------------------------------------------
// Wave-tiled SpMV: the same idea with a WAVE as the unit of work.  Each 64-lane
// wave owns tiles of <= 64 consecutive rows / <= 510 nonzeros, stages the
// products in its private 4 KiB LDS slice and sums one row per lane.  There is no
// workgroup barrier in the loop (LDS operations of one wave complete in order),
// so the four waves of a workgroup -- and the 32 of a CU -- drift apart and keep
// loads in flight while others are in their LDS phase.
// NT: matrix entries are read once per SpMV; loading them non-temporally keeps
// them from evicting the x planes that neighbouring tiles re-read from L2.
// ---------------------------------------------------------------------------

typedef double v2d __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));

template <typename T, bool NT>
__device__ __forceinline__ T stream_load(const T *p)
{
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int kWavePairs = kWaveTileNnz / 128;  // 16-byte pairs per lane per tile (4)

template <int MODE, bool NT>
__global__ __launch_bounds__(kBlock) void spmv_wave_kernel(CsrView A, SpmvArgs a)
{
    // every SpMV variant rounds each product before it is added (no FMA contraction), so
    // that all variants -- and the sequential CPU oracle -- produce the same bits
#pragma clang fp contract(off)
    __shared__ double prod_all[kBlock / 64][kWaveTileNnz + 2];
    __shared__ double red[4];
    if (MODE == kSpmvDot || MODE == kSpmvResidInit) {
        if (a.stop_iter && a.it >= *a.stop_iter) return;
    }
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    double *prod = prod_all[wave];
    const int xcd = blockIdx.x % kXcds;
    const int slot = (blockIdx.x / kXcds) * (kBlock / 64) + wave;
    const int per_xcd = (gridDim.x / kXcds) * (kBlock / 64);
    const int chunk = (A.nwtiles + kXcds - 1) / kXcds;
    double acc0 = 0.0, acc1 = 0.0;

    for (int t = slot; t < chunk; t += per_xcd) {
        const int tile = xcd * chunk + t;
        if (tile >= A.nwtiles) break;
        const int r0 = A.wtile_row[tile], r1 = A.wtile_row[tile + 1];
        const int s = A.rp[r0], e = A.rp[r1];
        const int cnt = e - s;
        double sum = 0.0;
        int row = r0 + lane;
        bool have_row = false;
        if (cnt <= kWaveTileNnz - 2) {
            const int s2 = s & ~1;
            int b0 = 0, b1 = 0;
            if (row < r1) {
                b0 = A.rp[row] - s2;
                b1 = A.rp[row + 1] - s2;
            }
            v2d v[kWavePairs];
            v2i c[kWavePairs];
#pragma unroll
            for (int k = 0; k < kWavePairs; ++k) {
                const int idx = s2 + 2 * (lane + 64 * k);
                if (idx < e) {
                    v[k] = stream_load<v2d, NT>(reinterpret_cast<const v2d *>(A.val + idx));
                    c[k] = stream_load<v2i, NT>(reinterpret_cast<const v2i *>(A.col + idx));
                }
            }
#pragma unroll
            for (int k = 0; k < kWavePairs; ++k) {
                const int idx = s2 + 2 * (lane + 64 * k);
                if (idx < e) {
                    v2d pr;
                    pr.x = v[k].x * a.x[c[k].x];
                    pr.y = v[k].y * a.x[c[k].y];
                    *reinterpret_cast<v2d *>(&prod[2 * (lane + 64 * k)]) = pr;
                }
            }
            wave_lds_sync();
            if (row < r1) {
                have_row = true;
                for (int j = b0; j < b1; ++j) sum += prod[j];
            }
            wave_lds_sync();
        } else {
            // a single row longer than a wave tile: the wave reduces it
            double part = 0.0;
            for (int i = lane; i < cnt; i += 64) part += __dmul_rn(A.val[s + i], a.x[A.col[s + i]]);
            part = wave_sum(part);
            row = r0;
            if (lane == 0) {
                have_row = true;
                sum = part;
            }
        }
        if (have_row) {
            if (MODE == kSpmvPlain) {
                a.y[row] = (a.beta == 0.0) ? a.alpha * sum : a.alpha * sum + a.beta * a.y[row];
            } else if (MODE == kSpmvDot) {
                a.y[row] = sum;
                acc0 += a.x[row] * sum;
            } else if (MODE == kSpmvResidInit) {
                const double r = a.b[row] - sum;
                const double z = a.dinv ? a.dinv[row] * r : r;
                a.y[row] = r;
                a.p[row] = z;
                acc0 += r * z;
                acc1 += r * r;
            } else {  // kSpmvResidNorm
                if (row < a.row_limit) {
                    const double r = a.b[row] - sum;
                    acc1 += r * r;
                }
            }
        }
    }
    if (MODE != kSpmvPlain) {
        const double s0 = block_sum(acc0, red);
        const double s1 = block_sum(acc1, red);
        if (threadIdx.x == 0) {
            a.partials[blockIdx.x] = s0;
            a.partials[gridDim.x + blockIdx.x] = s1;
        }
    }
}

// Baseline for A/B runs: one row per lane, no staging (what a direct port of a
// row-parallel CPU loop would do).  Only the plain mode.
__global__ __launch_bounds__(kBlock) void spmv_rowlane_kernel(CsrView A, SpmvArgs a)
{
    // every SpMV variant rounds each product before it is added (no FMA contraction), so
    // that all variants -- and the sequential CPU oracle -- produce the same bits
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x; row < A.nrows; row += stride) {
        double sum = 0.0;
        for (int j = A.rp[row]; j < A.rp[row + 1]; ++j) sum += A.val[j] * a.x[A.col[j]];
        a.y[row] = (a.beta == 0.0) ? a.alpha * sum : a.alpha * sum + a.beta * a.y[row];
    }
}

// ---------------------------------------------------------------------------
// The stream kernel as it stood before its tile pipeline moved to csrc/stream_pipeline.hpp (the macro form, two
// register sets pasted into the step by name), frozen here with its measurement bits: the product's
// spmv_stream_kernel has none.  Findings: profiles/r03_stream_ablate.txt, DESIGN.md section 3.
// ABL (variants 80 + ABL of schwz_csr_spmv): bit 0 no y store, bit 1 no x gather, bit 2 no
// row-pointer loads (7-entry rows assumed), bit 3 y stored into a 256 KiB window (the stores are issued, the
// bytes stay in L2), bit 4 x gathered from a 512 KiB window (the gathers are issued and hit L2), bit 5 the y
// store of a tile issued after the NEXT tile's gathers (the in-order vmcnt wait for those gathers then does
// not wait for the store's acknowledgement)
// ---------------------------------------------------------------------------
template <int MODE, int CAP, int ABL = 0, bool NTY = false>
__global__ __launch_bounds__(kBlock) void spmv_stream_ablate_kernel(CsrView A, SpmvArgs a)
{
#pragma clang fp contract(off)
    // the tile's values and columns as stored (16-byte aligned window of <= kTileNnz entries, + what the
    // masked reads of the last rows may touch)
    __shared__ __attribute__((aligned(16))) double vals[kTileNnz + 4 + CAP];
    __shared__ __attribute__((aligned(16))) int cols[kTileNnz + 4 + CAP];
    __shared__ int rstart[kBlock + 1];  // first entry of every row of the tile (window-relative)
    __shared__ double red[4];
    if (MODE == kSpmvDot || MODE == kSpmvResidInit) {
        if (a.stop_iter && a.it >= *a.stop_iter) return;
    }
    const int tid = threadIdx.x;
    const int xcd = blockIdx.x % kXcds;
    const int slot = blockIdx.x / kXcds;
    const int per_xcd = gridDim.x / kXcds;
    // an XCD's tile sequence: block-cyclic, or the explicit one of wide planes (CsrView::stream_order: entries past
    // the end are -1, mapped to ntiles = "no tile" here); read through the scalar cache
    typedef const int __attribute__((address_space(4))) *const_order;
    const const_order sorder = (const_order)(uintptr_t)A.stream_order;
    const int nslots = sorder ? A.stream_nper : xcd_slots(A);
    const int sh = A.xcd_shift;
    auto tile_at = [&](int j) -> int {
        if (sorder) {
            const int t = sorder[(int64_t)xcd * A.stream_nper + j];
            return t < 0 ? A.ntiles : t;
        }
        return ((j >> sh) << (sh + 3)) + (xcd << sh) + (j & (A.xcd_block - 1));
    };
    // tiles of this workgroup: k = 0 .. ntw - 1 (past-the-end slots only occur at the tail of the deal)
    // a.seq > 0: a workgroup takes a.seq CONSECUTIVE slots of its XCD's sequence and ends; the grid covers the
    // matrix once and the dispatch order keeps the active rows a compact window
    const int seq = a.seq;
    auto slot_at = [&](int k) -> int { return seq ? slot * seq + k : slot + k * per_xcd; };
    int ntw = seq ? max(0, min(seq, nslots - slot * seq)) : (slot < nslots ? (nslots - slot + per_xcd - 1) / per_xcd : 0);
    while (ntw > 0 && tile_at(slot_at(ntw - 1)) >= A.ntiles) --ntw;
    // partial-sum slots the consumer folds (a.part_stride of them per bank) beyond this launch's grid
    if (MODE != kSpmvPlain && blockIdx.x == 0)
        for (int i = (int)gridDim.x + tid; i < a.part_stride; i += kBlock) a.partials[i] = a.partials[a.part_stride + i] = 0.0;
    // the masked reads of a tile's last rows may run up to CAP entries past the window: keep that tail finite
    // and inside x (it is never summed, but its columns are gathered)
    if (tid < 4 + CAP) {
        vals[kTileNnz + tid] = 0.0;
        cols[kTileNnz + tid] = 0;
    }
    double acc0 = 0.0, acc1 = 0.0;
    if (ntw > 0) {
        typedef const int __attribute__((address_space(4))) *const_ints;
        const const_ints trow = (const_ints)(uintptr_t)A.tile_row;
        const const_ints tnz = (const_ints)(uintptr_t)A.tile_nz;
        struct Meta {
            int r0, r1, s, e;
        };
        auto meta = [&](int k) -> Meta {
            // beyond the workgroup's last tile: loaded (no branch in the loop), never computed -- one quad and
            // one row of the last tile, so that every such load instruction touches a single line
            const int t = tile_at(slot_at(min(k, ntw - 1)));
            const bool past = k >= ntw;
            const int r0 = trow[t], s0 = tnz[t];
            return Meta{r0, past ? r0 + 1 : trow[t + 1], s0, past ? s0 : tnz[t + 1]};
        };
        // Two register sets (tiles k and k + 1 in flight / landed), named scalars and native vectors pasted
        // into the step by macro: as members of a struct passed to a lambda they stayed in scratch memory
        // (the allocas were not promoted), which doubled the kernel time.
        typedef double vd2 __attribute__((ext_vector_type(2)));
        typedef int vi4 __attribute__((ext_vector_type(4)));
        const double *const dinv = a.dinv ? a.dinv : a.b;  // a valid address either way (the value is selected away)
#define SCHWZ_STREAM_ISSUE(M, P)                                                                     \
    {                                                                                                \
        const int s2_ = (M).s & ~3;                                                                  \
        const int last_ = max(((M).e - 1) & ~3, s2_);                                                \
        const int i0_ = min(s2_ + 4 * tid, last_), i1_ = min(s2_ + 4 * (tid + kBlock), last_);       \
        if (ABL & 64) {                                                                              \
            P##v0 = __builtin_nontemporal_load(reinterpret_cast<const vd2 *>(A.val + i0_));          \
            P##v1 = __builtin_nontemporal_load(reinterpret_cast<const vd2 *>(A.val + i0_ + 2));      \
            P##c0 = __builtin_nontemporal_load(reinterpret_cast<const vi4 *>(A.col + i0_));          \
            P##v2 = __builtin_nontemporal_load(reinterpret_cast<const vd2 *>(A.val + i1_));          \
            P##v3 = __builtin_nontemporal_load(reinterpret_cast<const vd2 *>(A.val + i1_ + 2));      \
            P##c1 = __builtin_nontemporal_load(reinterpret_cast<const vi4 *>(A.col + i1_));          \
        } else {                                                                                     \
            P##v0 = *reinterpret_cast<const vd2 *>(A.val + i0_);                                     \
            P##v1 = *reinterpret_cast<const vd2 *>(A.val + i0_ + 2);                                 \
            P##c0 = *reinterpret_cast<const vi4 *>(A.col + i0_);                                     \
            P##v2 = *reinterpret_cast<const vd2 *>(A.val + i1_);                                     \
            P##v3 = *reinterpret_cast<const vd2 *>(A.val + i1_ + 2);                                 \
            P##c1 = *reinterpret_cast<const vi4 *>(A.col + i1_);                                     \
        }                                                                                            \
        const int rowc_ = min((M).r0 + tid, (M).r1 - 1);                                             \
        /* ONE row-pointer load per lane: the end of a row is the start of the next lane's, handed */ \
        /* over through LDS in the step; the tile's last row ends where the tile does (M.e) */      \
        P##b0 = (ABL & 4) ? 7 * tid : A.rp[rowc_] - s2_;                                             \
        P##o0 = P##o1 = 0.0;                                                                         \
        if (MODE == kSpmvDot) P##o0 = a.x[rowc_];                                                    \
        if (MODE == kSpmvResidInit || MODE == kSpmvResidNorm) P##o0 = a.b[rowc_];                   \
        if (MODE == kSpmvResidInit) P##o1 = dinv[rowc_];                                             \
    }
        // One tile: set P holds its stream on entry and the stream of tile MN (two tiles on) on exit.  The
        // entries go to LDS as they are stored; then a lane IS a row: entry j of 64 consecutive rows per
        // gather instruction (for a stencil: one contiguous run of x), products rounded one by one and
        // added in CSR order.  The next stream is requested AFTER the first eight gathers (the scheduling
        // barriers keep hipcc from moving it up), so that waiting for them -- an in-order counter -- does
        // not wait for it.  The last two steps of a workgroup request its last tile again: no branch.
        // (Keeping the gathered operands of a tile for a step and summing one step later -- a whole step of
        // slack for the gathers, 126-157 registers -- measured the same: the launch is not bound by the
        // latency of its gathers.)
#define SCHWZ_STREAM_STEP(M, MN, P)                                                                  \
    {                                                                                                \
        const int b0 = P##b0;                                                                        \
        const double o0 = P##o0, o1 = P##o1;                                                         \
        lds_barrier(); /* every lane is done with the previous tile's entries */                     \
        rstart[tid] = b0;                                                                            \
        *reinterpret_cast<vd2 *>(&vals[4 * tid]) = P##v0;                                            \
        *reinterpret_cast<vd2 *>(&vals[4 * tid + 2]) = P##v1;                                        \
        *reinterpret_cast<vi4 *>(&cols[4 * tid]) = P##c0;                                            \
        *reinterpret_cast<vd2 *>(&vals[4 * (tid + kBlock)]) = P##v2;                                 \
        *reinterpret_cast<vd2 *>(&vals[4 * (tid + kBlock) + 2]) = P##v3;                             \
        *reinterpret_cast<vi4 *>(&cols[4 * (tid + kBlock)]) = P##c1;                                 \
        lds_barrier();                                                                               \
        const int b1 = (M).r0 + tid + 1 < (M).r1 ? rstart[tid + 1] : (M).e - ((M).s & ~3);          \
        double sum = 0.0;                                                                            \
        _Pragma("unroll") for (int j0 = 0; j0 < CAP; j0 += 8)                                        \
        {                                                                                            \
            double vv[8], xx[8];                                                                     \
            int cc[8];                                                                               \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                                            \
            {                                                                                        \
                vv[j] = vals[b0 + j0 + j];                                                           \
                cc[j] = cols[b0 + j0 + j];                                                           \
            }                                                                                        \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                                            \
                xx[j] = (ABL & 2) ? (double)cc[j] : a.x[(ABL & 16) ? (cc[j] & 0xFFFF) : cc[j]];      \
            if (j0 == 0) {                                                                           \
                __builtin_amdgcn_sched_barrier(0);                                                   \
                if (ABL & 32) a.y[(ABL & 8) ? (prow & 0x7FFF) : prow] = psum;                        \
                SCHWZ_STREAM_ISSUE(MN, P)                                                            \
                __builtin_amdgcn_sched_barrier(0);                                                   \
            }                                                                                        \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                                            \
            {                                                                                        \
                const double pv = vv[j] * xx[j];                                                     \
                sum += (b0 + j0 + j < b1) ? pv : 0.0;                                                \
            }                                                                                        \
        }                                                                                            \
        const int rowc = min((M).r0 + tid, (M).r1 - 1);                                              \
        const bool mine = (M).r0 + tid < (M).r1;                                                     \
        if (MODE == kSpmvPlain) {                                                                    \
            if (ABL & 1)                                                                             \
                acc0 += sum;                                                                         \
            else if (ABL & 32) {                                                                     \
                psum = a.alpha * sum;                                                                \
                prow = rowc;                                                                         \
            } else if ((ABL & 128) || NTY)                                                           \
                __builtin_nontemporal_store(a.alpha * sum, a.y + rowc);                              \
            else                                                                                     \
                a.y[(ABL & 8) ? (rowc & 0x7FFF) : rowc] = a.alpha * sum;                             \
        } else if (MODE == kSpmvDot) {                                                               \
            if (NTY)                                                                                 \
                __builtin_nontemporal_store(sum, a.y + rowc);                                        \
            else                                                                                     \
                a.y[rowc] = sum;                                                                     \
            const double t = o0 * sum;                                                               \
            acc0 += mine ? t : 0.0;                                                                  \
        } else if (MODE == kSpmvResidInit) {                                                         \
            const double r = o0 - sum;                                                               \
            const double z = a.dinv ? o1 * r : r;                                                    \
            a.y[rowc] = r;                                                                           \
            a.p[rowc] = z;                                                                           \
            const double t0 = r * z, t1 = r * r;                                                     \
            acc0 += mine ? t0 : 0.0;                                                                 \
            acc1 += mine ? t1 : 0.0;                                                                 \
        } else { /* kSpmvResidNorm */                                                                \
            const double r = o0 - sum;                                                               \
            const double t1 = r * r;                                                                 \
            acc1 += (mine && rowc < a.row_limit) ? t1 : 0.0;                                         \
        }                                                                                            \
    }
        vd2 Av0, Av1, Av2, Av3, Bv0, Bv1, Bv2, Bv3;
        vi4 Ac0, Ac1, Bc0, Bc1;
        int Ab0, Bb0;
        double Ao0, Ao1, Bo0, Bo1;
        Meta m0 = meta(0), m1 = meta(1);
        // delayed store (ABL bit 5): the first step stores 0.0 to the rows its own tile stores again one step
        // later (same lane, same address, program order)
        double psum = 0.0;
        int prow = min(m0.r0 + tid, m0.r1 - 1);
        SCHWZ_STREAM_ISSUE(m0, A)
        SCHWZ_STREAM_ISSUE(m1, B)
        Meta m2 = meta(2), m3 = meta(3);
        int k = 0;
        for (; k + 1 < ntw; k += 2) {
            SCHWZ_STREAM_STEP(m0, m2, A)
            SCHWZ_STREAM_STEP(m1, m3, B)
            m0 = m2;
            m1 = m3;
            m2 = meta(k + 4);
            m3 = meta(k + 5);
        }
        if (k < ntw) SCHWZ_STREAM_STEP(m0, m2, A)
        if ((ABL & 32) && !(ABL & 1)) a.y[(ABL & 8) ? (prow & 0x7FFF) : prow] = psum;
#undef SCHWZ_STREAM_STEP
#undef SCHWZ_STREAM_ISSUE
    }
    if (MODE == kSpmvPlain && (ABL & 1)) {
        if (acc0 == 123.456) a.y[tid] = acc0;  // keeps the sums alive
    }
    if (MODE != kSpmvPlain) {
        // (one partial sum per WAVE instead -- no barrier at the end of a short-lived workgroup's life, four times
        // the slots to fold -- measured the same step time, round 3)
        const double s0 = block_sum(acc0, red);
        const double s1 = MODE == kSpmvDot ? 0.0 : block_sum(acc1, red);
        if (tid == 0) {
            a.partials[blockIdx.x] = s0;
            a.partials[a.part_stride + blockIdx.x] = s1;
        }
    }
}

// measurement builds of the plain mode (tools/stream_ablate.py, tools/r03_stream_probe.py)
static int launch_spmv_stream_ablate(const CsrView &A, const SpmvArgs &a, int abl, hipStream_t s)
{
    if (A.stream_cap == 0 || A.stream_cap > 8 || !A.tile_nz || A.tile_order) {
        set_error("schwz_csr_spmv: the stream ablation builds need a matrix the stream kernel takes (rows <= 8 entries)");
        return SCHWZ_ERR_INVALID;
    }
    const char *ge = std::getenv("SCHWZ_STREAM_GRID");
    int g = ge ? std::atoi(ge) : kMaxGrid;
    g = std::max(kXcds, std::min(g, kMaxGrid) / kXcds * kXcds);
    SpmvArgs b = a;
    const char *se = std::getenv("SCHWZ_STREAM_SEQ");
    b.seq = se ? std::max(0, std::atoi(se)) : 0;
    if (b.seq) g = kXcds * ((stream_slots(A) + b.seq - 1) / b.seq);
    switch (abl) {
#define SCHWZ_ABL(W) \
    case W: hipLaunchKernelGGL((spmv_stream_ablate_kernel<kSpmvPlain, 8, W>), dim3(g), dim3(kBlock), 0, s, A, b); break;
        SCHWZ_ABL(0) SCHWZ_ABL(1) SCHWZ_ABL(2) SCHWZ_ABL(3) SCHWZ_ABL(4) SCHWZ_ABL(5) SCHWZ_ABL(6) SCHWZ_ABL(7)
        SCHWZ_ABL(8) SCHWZ_ABL(16) SCHWZ_ABL(24) SCHWZ_ABL(32) SCHWZ_ABL(40) SCHWZ_ABL(48) SCHWZ_ABL(56)
        SCHWZ_ABL(64) SCHWZ_ABL(128) SCHWZ_ABL(192)
    default: set_error("schwz_csr_spmv: no such stream ablation build"); return SCHWZ_ERR_INVALID;
#undef SCHWZ_ABL
    }
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

static int launch_spmv_probe(const CsrView &A, int mode, const SpmvArgs &a, int variant, int grid, hipStream_t s)
{
#define SCHWZ_LAUNCH_WAVE(NTV)                                                                          \
    switch (mode) {                                                                                    \
    case kSpmvPlain:                                                                                   \
        hipLaunchKernelGGL((spmv_wave_kernel<kSpmvPlain, NTV>), dim3(wgrid), dim3(kBlock), 0, s, A, a); \
        break;                                                                                         \
    case kSpmvDot:                                                                                     \
        hipLaunchKernelGGL((spmv_wave_kernel<kSpmvDot, NTV>), dim3(wgrid), dim3(kBlock), 0, s, A, a);   \
        break;                                                                                         \
    case kSpmvResidInit:                                                                               \
        hipLaunchKernelGGL((spmv_wave_kernel<kSpmvResidInit, NTV>), dim3(wgrid), dim3(kBlock), 0, s, A, a); \
        break;                                                                                         \
    default:                                                                                           \
        hipLaunchKernelGGL((spmv_wave_kernel<kSpmvResidNorm, NTV>), dim3(wgrid), dim3(kBlock), 0, s, A, a); \
        break;                                                                                         \
    }
    if (variant >= 80) {
        if (mode != kSpmvPlain) {
            set_error("schwz_csr_spmv: the stream ablation builds are y = A x only");
            return SCHWZ_ERR_INVALID;
        }
        return launch_spmv_stream_ablate(A, a, variant - 80, s);
    }
    if (variant >= 10 && variant < 74) {
        if (mode != kSpmvPlain) {
            set_error("schwz_csr_spmv: the ablation builds are y = A x only");
            return SCHWZ_ERR_INVALID;
        }
        switch (variant - 10) {
#define SCHWZ_ABL(W) \
    case W: hipLaunchKernelGGL(spmv_ablate_kernel<W>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
            SCHWZ_ABL(0) SCHWZ_ABL(1) SCHWZ_ABL(2) SCHWZ_ABL(3) SCHWZ_ABL(4) SCHWZ_ABL(5) SCHWZ_ABL(6) SCHWZ_ABL(7)
            SCHWZ_ABL(8) SCHWZ_ABL(9) SCHWZ_ABL(10) SCHWZ_ABL(11) SCHWZ_ABL(12) SCHWZ_ABL(13) SCHWZ_ABL(14) SCHWZ_ABL(15)
            SCHWZ_ABL(16) SCHWZ_ABL(32) SCHWZ_ABL(48) SCHWZ_ABL(36)
#undef SCHWZ_ABL
        }
    } else if (variant == 3 || variant == 5) {
        const int wgrid = spmv_grid(A, variant);
        if (variant == 3) {
            SCHWZ_LAUNCH_WAVE(false)
        } else {
            SCHWZ_LAUNCH_WAVE(true)
        }
    } else if (variant == 1) {
        if (mode != kSpmvPlain) {
            set_error("schwz_csr_spmv: variant 1 is y = A x only");
            return SCHWZ_ERR_INVALID;
        }
        hipLaunchKernelGGL(spmv_rowlane_kernel, dim3(kMaxGrid), dim3(kBlock), 0, s, A, a);
    } else if (variant == 4) {
        switch (mode) {
        case kSpmvPlain: hipLaunchKernelGGL(spmv_pipe_kernel<kSpmvPlain>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
        case kSpmvDot: hipLaunchKernelGGL(spmv_pipe_kernel<kSpmvDot>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
        case kSpmvResidInit: hipLaunchKernelGGL(spmv_pipe_kernel<kSpmvResidInit>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
        case kSpmvResidDual: hipLaunchKernelGGL(spmv_pipe_kernel<kSpmvResidDual>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
        default: hipLaunchKernelGGL(spmv_pipe_kernel<kSpmvResidNorm>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
        }
    } else {  // variant 2
        switch (mode) {
        case kSpmvPlain: hipLaunchKernelGGL(spmv_tiled_kernel<kSpmvPlain>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
        case kSpmvDot: hipLaunchKernelGGL(spmv_tiled_kernel<kSpmvDot>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
        case kSpmvResidInit: hipLaunchKernelGGL(spmv_tiled_kernel<kSpmvResidInit>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
        default: hipLaunchKernelGGL(spmv_tiled_kernel<kSpmvResidNorm>, dim3(grid), dim3(kBlock), 0, s, A, a); break;
        }
    }
#undef SCHWZ_LAUNCH_WAVE
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

// linking this file into the library is what switches the measurement variants on
static const bool g_registered = [] {
    g_spmv_probe_hook = launch_spmv_probe;
    return true;
}();

}  // namespace schwz
