// Plain-CSR SpMV as a straight-line software pipeline (variants 0 / 6 on matrices whose rows hold at most 32
// entries): the same tiles, the same products and the same per-row summation order as spmv_tiled2_kernel
// (spmv_csr.hip) -- the same bits --, but nothing in a workgroup's tile loop waits for a chain of dependent
// loads any more.
//
// What bounded spmv_tiled2_kernel (0.37 ms at 256^3 = 0.58 of the 8 TB/s peak while its matrix stream alone
// runs at 6.05 TB/s): per tile a workgroup went through tile table -> row pointers -> val / col -> x gather ->
// LDS -> row sums, five dependent memory round trips of 2-3 us each under load, with 8 workgroups per CU to
// hide them, and every guarded load (`if (row < r1)`) made hipcc fall back to `s_waitcnt vmcnt(0)`.  The tile
// pipeline that replaces the chain is stream_pipeline.hpp; this file holds the fused epilogues, the fold of the
// partial sums and the choice of the grid.
// Workgroups are SHORT-LIVED (round 3): a workgroup takes a.seq = 3 consecutive tiles of its XCD's sequence and
// ends, and the grid covers the matrix once.  The round-2 form (persistent workgroups striding through the
// sequence, a.seq = 0, SCHWZ_STREAM_SEQ=0) lets the workgroups drift apart: the rows in flight spread over the
// whole sweep, the x lines neighbouring tiles share are gone from the 4 MiB L2 (a line lives ~5 us there at
// this stream rate) before the neighbour asks, and the y stores reach memory as scattered 2 KiB pieces.  With
// workgroups that end after four tiles the dispatch order keeps the active rows a compact moving window:
// 0.359 -> 0.322 ms at 256^3 and 0.380 -> 0.320 ms on the 512 x 512 x 64 slab together with non-temporal y
// stores (profiles/r03_stream_seq.txt; two tiles per workgroup pay too much pipeline fill, eight drift again).
// The y values are the same bits as before; the partial sums of the fused dots are per workgroup, and a grid
// beyond the kMaxGrid slots the consumers fold is reduced to them by spmv_stream_fold_kernel in a fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "schwz_internal.hpp"
#include "device_utils.hpp"
#include "stream_pipeline.hpp"

namespace schwz {

template <int MODE, int CAP, bool NTY = false>
__global__ __launch_bounds__(kBlock) void spmv_stream_kernel(CsrView A, SpmvArgs a)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    if (MODE == kSpmvDot || MODE == kSpmvResidInit) {
        if (a.stop_iter && a.it >= *a.stop_iter) return;
    }
    const int tid = threadIdx.x;
    // partial-sum slots the consumer folds (a.part_stride of them per bank) beyond this launch's grid
    if (MODE != kSpmvPlain && blockIdx.x == 0)
        for (int i = (int)gridDim.x + tid; i < a.part_stride; i += kBlock) a.partials[i] = a.partials[a.part_stride + i] = 0.0;
    double acc0 = 0.0, acc1 = 0.0;
    const double *const dinv = a.dinv ? a.dinv : a.b;  // a valid address either way (the value is selected away)
    struct Ops {
        double o0, o1;
    };
    auto load = [&](int rowc) -> Ops {
        Ops o{0.0, 0.0};
        if (MODE == kSpmvDot) o.o0 = a.x[rowc];
        if (MODE == kSpmvResidInit || MODE == kSpmvResidNorm) o.o0 = a.b[rowc];
        if (MODE == kSpmvResidInit) o.o1 = dinv[rowc];
        return o;
    };
    // lanes past the tile's last row store the same value to the same address again and add +0.0 to the sums
    auto row = [&](double sum, const Ops &o, int rowc, bool mine) {
        if (MODE == kSpmvPlain) {
            if (NTY)
                __builtin_nontemporal_store(a.alpha * sum, a.y + rowc);
            else
                a.y[rowc] = a.alpha * sum;
        } else if (MODE == kSpmvDot) {
            if (NTY)
                __builtin_nontemporal_store(sum, a.y + rowc);
            else
                a.y[rowc] = sum;
            const double t = o.o0 * sum;
            acc0 += mine ? t : 0.0;
        } else if (MODE == kSpmvResidInit) {
            const double r = o.o0 - sum;
            const double z = a.dinv ? o.o1 * r : r;
            a.y[rowc] = r;
            a.p[rowc] = z;
            const double t0 = r * z, t1 = r * r;
            acc0 += mine ? t0 : 0.0;
            acc1 += mine ? t1 : 0.0;
        } else {  // kSpmvResidNorm
            const double r = o.o0 - sum;
            const double t1 = r * r;
            acc1 += (mine && rowc < a.row_limit) ? t1 : 0.0;
        }
    };
    SCHWZ_STREAM_PIPELINE(A, CAP, double, A.val, a.x, a.seq, true, Ops, load, row)
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

// Folds the partial sums of a launch (`nin` per bank: one per workgroup or per wave, two banks `nin` apart) into
// the `nout` slots per bank the consumers read.  Slot i takes the partial sums i, i + nout, i + 2 nout, ...; eight
// adjacent lanes share a slot (lane l sums every eighth of them, four loads in flight, then a fixed xor tree), so the
// launch is a few dependent L2 round trips long whatever `nin` is.  Fixed order: reproducible bit for bit.
constexpr int kFoldSub = 8;

template <int MODE>
__global__ __launch_bounds__(kBlock) void spmv_stream_fold_kernel(const double *__restrict__ in, int nin,
                                                                  double *__restrict__ out, int nout,
                                                                  const int *stop_iter, int it)
{
    if (MODE == kSpmvDot || MODE == kSpmvResidInit) {
        if (stop_iter && it >= *stop_iter) return;
    }
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const int i = min(t / kFoldSub, nout - 1), l = t % kFoldSub;  // surplus lanes repeat the last slot (whole groups of 8)
    constexpr bool two = MODE != kSpmvDot;                        // the p.q launch fills one bank
    const int64_t step = (int64_t)nout * kFoldSub;
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t j = i + (int64_t)nout * l; j < nin; j += 4 * step) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t ju = j + u * step;
            const bool in_range = ju < nin;
            const double a0 = in[in_range ? ju : j];
            s0[u] += in_range ? a0 : 0.0;
            if (two) {
                const double a1 = in[nin + (in_range ? ju : j)];
                s1[u] += in_range ? a1 : 0.0;
            }
        }
    }
    double v0 = (s0[0] + s0[1]) + (s0[2] + s0[3]);
    double v1 = (s1[0] + s1[1]) + (s1[2] + s1[3]);
#pragma unroll
    for (int m = 1; m < kFoldSub; m <<= 1) {
        v0 += __shfl_xor(v0, m, 64);
        if (two) v1 += __shfl_xor(v1, m, 64);
    }
    if (l == 0 && t / kFoldSub < nout) {
        out[i] = v0;
        out[nout + i] = two ? v1 : 0.0;
    }
}

// tiles per short-lived workgroup (SCHWZ_STREAM_SEQ; 0: the persistent form) and whether y leaves with
// non-temporal stores (SCHWZ_STREAM_NTY: 0 never, 1 y = A x only, 2 the q = A p of the CG iteration as well -- the
// default: 0.5-1 % of the plain-CSR step on two boxes, profiles/r03_plainloop_ab.txt)
static int stream_seq_max()
{
    static const int v = [] {
        const char *e = std::getenv("SCHWZ_STREAM_SEQ");
        return e ? std::max(0, std::min(std::atoi(e), 64)) : 3;
    }();
    return v;
}

static int stream_nty()
{
    static const int v = [] {
        const char *e = std::getenv("SCHWZ_STREAM_NTY");
        return e ? std::atoi(e) : 2;
    }();
    return v;
}

// Launches the stream kernel where it applies; *done = false leaves the launch to spmv_tiled2_kernel.
int launch_spmv_stream(const CsrView &A, int mode, const SpmvArgs &a, int grid, hipStream_t s, bool *done)
{
    *done = false;
    static const bool on = [] {
        const char *e = std::getenv("SCHWZ_SPMV_STREAM");
        return !(e && e[0] == '0');
    }();
    if (!on || !stream_takes(A)) return SCHWZ_OK;
    if (!(mode == kSpmvPlain || mode == kSpmvDot || mode == kSpmvResidInit || mode == kSpmvResidNorm)) return SCHWZ_OK;
    if (mode == kSpmvPlain && a.beta != 0.0) return SCHWZ_OK;
    SpmvArgs b = a;
    b.part_stride = grid;
    // short-lived workgroups (stream_seq_max() consecutive tiles each) once the matrix has four tiles per
    // workgroup of the persistent grid (2 M rows): below that launches, not memory, set the pace
    int launch_grid = grid;
    bool fold = false;
    const int seq = stream_seq_max();
    if (seq && A.ntiles >= 4 * kMaxGrid) {
        const int g = kXcds * ((stream_slots(A) + seq - 1) / seq);
        if (mode == kSpmvPlain || (a.stream_part && g <= A.stream_part_cap)) {
            b.seq = seq;
            launch_grid = g;
            if (mode != kSpmvPlain) {
                fold = true;
                b.partials = a.stream_part;
                b.part_stride = g;
            }
        }
    }
    const bool nty = b.seq && ((mode == kSpmvPlain && stream_nty() >= 1) || (mode == kSpmvDot && stream_nty() >= 2));
    auto launch = [&](auto m, auto cap) {
        constexpr int M = decltype(m)::value, C = decltype(cap)::value;
        if (nty)
            hipLaunchKernelGGL((spmv_stream_kernel<M, C, true>), dim3(launch_grid), dim3(kBlock), 0, s, A, b);
        else
            hipLaunchKernelGGL((spmv_stream_kernel<M, C, false>), dim3(launch_grid), dim3(kBlock), 0, s, A, b);
        if (fold)
            hipLaunchKernelGGL((spmv_stream_fold_kernel<M>), dim3((grid * kFoldSub + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                               (const double *)b.partials, b.part_stride, a.partials, grid, a.stop_iter, a.it);
    };
    stream_cap_dispatch(A, [&](auto cap) {
        switch (mode) {
        case kSpmvPlain: launch(std::integral_constant<int, kSpmvPlain>(), cap); break;
        case kSpmvDot: launch(std::integral_constant<int, kSpmvDot>(), cap); break;
        case kSpmvResidInit: launch(std::integral_constant<int, kSpmvResidInit>(), cap); break;
        default: launch(std::integral_constant<int, kSpmvResidNorm>(), cap); break;
        }
    });
    SCHWZ_HIP_TRY(hipGetLastError());
    *done = true;
    return SCHWZ_OK;
}

}  // namespace schwz
