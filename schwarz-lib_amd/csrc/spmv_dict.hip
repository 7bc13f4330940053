// Dictionary-coded CSR tiles: a lossless re-encoding of (val, col) built once at upload.
//
// Many matrices on this path (the Poisson stencils, FEM operators on regular meshes) repeat a
// handful of values and a handful of (column - row) offsets inside every run of 256 rows.  For
// each row tile whose entries use at most 256 distinct values and 256 distinct offsets the 12
// bytes per nonzero of CSR become 2: one byte indexing a per-tile value dictionary, one byte
// indexing a per-tile offset dictionary.
// Tiles that do not qualify keep using val/col.  The arithmetic is unchanged -- the same
// products are summed in the same (ascending column) order -- so results are bit-identical to
// the plain CSR kernels; only the HBM traffic differs.
//
// Kernel: the tile's codes (<= 4 KiB) and dictionaries are staged in LDS with coalesced loads;
// then ONE LANE PER ROW decodes its entries and gathers x.  Consecutive lanes hold consecutive
// rows, so for banded matrices each gather instruction reads one contiguous run of x (the k-th
// neighbour of 64 consecutive rows) instead of the ~20 scattered lines of an entry-parallel
// gather.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "coding_plan.hpp"
#include "device_utils.hpp"
#include "schwz_internal.hpp"

namespace schwz {

template <int MODE>
__global__ __launch_bounds__(kBlock) void spmv_dict_kernel(CsrView A, SpmvArgs a)
{
    // every SpMV variant rounds each product before it is added (no FMA contraction), so
    // that all variants -- and the sequential CPU oracle -- produce the same bits
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) uint16_t codes[kTileNnz + 8];
    __shared__ double vdict[kDictMax];
    __shared__ int ddict[kDictMax];
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

    for (int t = slot; t < chunk; t += per_xcd) {
        const int tile = xcd_tile(A, xcd, t);
        if (tile < 0) continue;
        const int r0 = A.tile_row[tile], r1 = A.tile_row[tile + 1];
        const int s = A.rp[r0], e = A.rp[r1];
        const int v0 = A.vdict_ptr[tile], nv = A.vdict_ptr[tile + 1] - v0;
        const int d0 = A.ddict_ptr[tile], nd = A.ddict_ptr[tile + 1] - d0;
        const int row = r0 + tid;
        const bool have_row = (r1 - r0 > 1) ? row < r1 : tid == 0;
        const bool dual_t = dual && (!A.tile_dual || A.tile_dual[tile]);
        double sum = 0.0, sum2 = 0.0;
        if (nd > 0) {
            // ---- coded tile ------------------------------------------------------------------
            const int s4 = s & ~3;  // 8-byte aligned window of 2-byte codes
            int b0 = 0, b1 = 0;
            if (row < r1) {
                b0 = A.rp[row] - s4;
                b1 = A.rp[row + 1] - s4;
            }
            const int last = max((e - 1) & ~3, s4);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int idx = min(s4 + 4 * (tid + kBlock * k), last);
                *reinterpret_cast<uint2 *>(&codes[4 * (tid + kBlock * k)]) =
                    *reinterpret_cast<const uint2 *>(A.code + idx);
            }
            if (tid < nv) vdict[tid] = A.vdict[v0 + tid];
            if (tid < nd) ddict[tid] = A.ddict[d0 + tid];
            lds_barrier();
            if (row < r1) {
                for (int j = b0; j < b1; j += kChunk) {
                    double v[kChunk], xg[kChunk], xg2[kChunk];
                    int c[kChunk];
                    const int jl = b1 - 1;
#pragma unroll
                    for (int k = 0; k < kChunk; ++k) {
                        const unsigned cd = codes[min(j + k, jl)];
                        v[k] = vdict[cd & 255u];
                        c[k] = row + ddict[cd >> 8];
                    }
#pragma unroll
                    for (int k = 0; k < kChunk; ++k) xg[k] = a.x[c[k]];
                    if (dual_t) {
#pragma unroll
                        for (int k = 0; k < kChunk; ++k) xg2[k] = a.x2[c[k]];
                    }
#pragma unroll
                    for (int k = 0; k < kChunk; ++k) {
                        // product rounded on its own (no FMA contraction): the plain CSR
                        // kernels round it when they stage it in LDS, and the two must agree
                        if (j + k < b1) {
                            sum += __dmul_rn(v[k], xg[k]);
                            if (dual_t) sum2 += __dmul_rn(v[k], xg2[k]);
                        }
                    }
                }
            }
            lds_barrier();
        } else if (r1 - r0 > 1) {
            // ---- raw tile: one lane per row straight from val/col --------------------------------
            if (row < r1) {
                for (int j = A.rp[row]; j < A.rp[row + 1]; ++j) {
                    const double vv = A.val[j];
                    const int cc = A.col[j];
                    sum += __dmul_rn(vv, a.x[cc]);
                    if (dual_t) sum2 += __dmul_rn(vv, a.x2[cc]);
                }
            }
        } else {
            // ---- a single long row: the whole workgroup reduces it ------------------------------
            double part = 0.0, part2 = 0.0;
            for (int i = s + tid; i < e; i += kBlock) {
                part += __dmul_rn(A.val[i], a.x[A.col[i]]);
                if (dual_t) part2 += __dmul_rn(A.val[i], a.x2[A.col[i]]);
            }
            sum = block_sum(part, red);
            if (dual_t) sum2 = block_sum(part2, red);
        }
        if (have_row) {
            const int rw = (r1 - r0 > 1) ? row : r0;
            if (MODE == kSpmvPlain) {
                a.y[rw] = (a.beta == 0.0) ? a.alpha * sum : a.alpha * sum + a.beta * a.y[rw];
            } else if (MODE == kSpmvDot) {
                a.y[rw] = sum;
                acc0 += a.x[rw] * sum;
            } else if (MODE == kSpmvResidInit || MODE == kSpmvResidDual) {
                const double bb = a.b[rw];
                const double r = bb - sum;
                const double z = a.dinv ? a.dinv[rw] * r : r;
                a.y[rw] = r;
                a.p[rw] = z;
                acc0 += r * z;
                acc1 += r * r;
                if (MODE == kSpmvResidDual && rw < a.row_limit) {
                    const double r2 = dual_t ? bb - sum2 : r;
                    acc2 += r2 * r2;
                }
            } else {  // kSpmvResidNorm
                if (rw < a.row_limit) {
                    const double r = a.b[rw] - sum;
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
        if (MODE == kSpmvResidDual) {
            const double s2v = block_sum(acc2, red);
            if (tid == 0) a.partials[2 * gridDim.x + blockIdx.x] = s2v;
        }
    }
}

int launch_spmv_dict(const CsrView &A, int mode, const SpmvArgs &a, int grid, hipStream_t s)
{
    switch (mode) {
    case kSpmvPlain:
        hipLaunchKernelGGL(spmv_dict_kernel<kSpmvPlain>, dim3(grid), dim3(kBlock), 0, s, A, a);
        break;
    case kSpmvDot:
        hipLaunchKernelGGL(spmv_dict_kernel<kSpmvDot>, dim3(grid), dim3(kBlock), 0, s, A, a);
        break;
    case kSpmvResidInit:
        hipLaunchKernelGGL(spmv_dict_kernel<kSpmvResidInit>, dim3(grid), dim3(kBlock), 0, s, A, a);
        break;
    case kSpmvResidDual:
        hipLaunchKernelGGL(spmv_dict_kernel<kSpmvResidDual>, dim3(grid), dim3(kBlock), 0, s, A, a);
        break;
    default:
        hipLaunchKernelGGL(spmv_dict_kernel<kSpmvResidNorm>, dim3(grid), dim3(kBlock), 0, s, A, a);
        break;
    }
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

// =============================================================================================
// Row-pattern coding: the second level of the same idea.  In a stencil-like matrix almost every
// row of a tile is one of a few (values, col - row offsets) sequences; coding the SEQUENCE costs
// one byte per ROW.  A tile's table of <= 64 patterns (<= 1024 entries) is staged in LDS, and
// because most tiles share one table (tables are de-duplicated at build time) a workgroup
// reloads it only when the table id changes -- the row loop then runs without any barrier:
// per row 1 byte of matrix, the coalesced x gathers, 8 bytes of y.  Summation order is the
// row's entry order, products rounded individually: bit-identical to the CSR kernels again.
// =============================================================================================

// (kPatMax, kPatEntries, kChunk, pat_stride: coding_plan.hpp, shared with the plan)

// One staged table entry: the value and the BYTE offset of the column relative to the row
// (col - row) * 8 (WIDE: col - row), read together by one ds_read_b128.  Pattern p starts at entry p * ls with
// ls = lmax rounded up to kChunk, so entry k of a chunk sits at an immediate offset; the padding
// entries are (0.0, 0): a lane past its row's length gathers x[row] and discards it.
struct __attribute__((aligned(16))) PatEntry {
    double val;
    int off8;
    int pad;
};

// NT: tiles a workgroup works on at a time (NT rows per lane; 2 was measured and is slower: the
// registers cost occupancy).  WIDE: x needs 64-bit offsets (>= 2^28 columns); otherwise the
// gathers use the scalar-base + 32-bit-lane-offset form.
template <int MODE, int NT, bool WIDE>
__global__ __launch_bounds__(kBlock) void spmv_pattern_kernel(CsrView A, SpmvArgs a)
{
#pragma clang fp contract(off)
    __shared__ PatEntry ptab[kPatEntries];
    __shared__ int plen[kPatMax];
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
    int cached = -1, ls = 0;  // staged table and its row stride

    auto stage_table = [&](int tb) {  // workgroup-uniform
        if (tb == cached) return;
        const int eoff = A.tbl_desc[4 * tb], loff = A.tbl_desc[4 * tb + 1];
        const int npat = A.tbl_desc[4 * tb + 2], lmax = A.tbl_desc[4 * tb + 3];
        ls = pat_stride(lmax);
        lds_barrier();  // everyone is done with the previous table
        for (int i = tid; i < npat * ls; i += kBlock) {
            const int pt = i / ls, k = i - pt * ls;
            PatEntry e;
            e.val = k < lmax ? A.tbl_val[eoff + pt * lmax + k] : 0.0;
            e.off8 = k < lmax ? A.tbl_delta[eoff + pt * lmax + k] * (WIDE ? 1 : 8) : 0;
            e.pad = 0;
            ptab[i] = e;
        }
        if (tid < npat) plen[tid] = A.tbl_len[loff + tid];
        lds_barrier();
        cached = tb;
    };
    auto xload = [&](const double *xv, int row, int off8) -> double {
        if (WIDE) return xv[(int64_t)row + off8];  // the entry holds col - row itself
        const uint32_t o = (uint32_t)row * 8u + (uint32_t)off8;
        return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(xv) + o);
    };
    // the row's own operands of the fused epilogue (requested ahead of the x gathers)
    auto own_load = [&](bool have, int rw, double &ox, double &ob, double &od, bool with_x) {
        ox = 0.0, ob = 0.0, od = 1.0;
        if (!have) return;
        if (MODE == kSpmvDot && with_x) ox = a.x[rw];
        if (MODE == kSpmvResidInit || MODE == kSpmvResidDual) ob = a.b[rw];
        if (MODE == kSpmvResidNorm && rw < a.row_limit) ob = a.b[rw];
        if ((MODE == kSpmvResidInit || MODE == kSpmvResidDual) && a.dinv) od = a.dinv[rw];
        if (MODE == kSpmvPlain && a.beta != 0.0) ob = a.y[rw];
    };
    auto epilogue = [&](int rw, double sum, double sum2, bool dual_t, double ox, double ob, double od) {
        if (MODE == kSpmvPlain) {
            a.y[rw] = (a.beta == 0.0) ? a.alpha * sum : a.alpha * sum + a.beta * ob;
        } else if (MODE == kSpmvDot) {
            a.y[rw] = sum;
            acc0 += ox * sum;
        } else if (MODE == kSpmvResidInit || MODE == kSpmvResidDual) {
            const double r = ob - sum;
            const double z = a.dinv ? od * r : r;
            a.y[rw] = r;
            a.p[rw] = z;
            acc0 += r * z;
            acc1 += r * r;
            if (MODE == kSpmvResidDual && rw < a.row_limit) {
                const double r2 = dual_t ? ob - sum2 : r;
                acc2 += r2 * r2;
            }
        } else {  // kSpmvResidNorm
            if (rw < a.row_limit) {
                const double r = ob - sum;
                acc1 += r * r;
            }
        }
    };
    // entries [j0, len) of the lane's pattern against vector xv, in entry order
    auto row_tail = [&](const double *xv, int row, int base, int len, int j0, double &sum) {
        for (int j = j0; j < len; j += kChunk) {
            double v[kChunk], xg[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                const PatEntry e = ptab[base + j + k];
                v[k] = e.val;
                xg[k] = xload(xv, row, e.off8);
            }
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                if (j + k < len) sum += v[k] * xg[k];
        }
    };
    // one tile on its own: any kind (pattern table, plain rows, one long row)
    auto one_tile = [&](int tile, int r0, int r1, int tb) {
        const int row = r0 + tid;
        const bool single = r1 - r0 == 1;
        const bool have_row = single ? tid == 0 : row < r1;
        const int rw = single ? r0 : row;
        const bool dual_t = dual && (!A.tile_dual || A.tile_dual[tile]);
        double ox, ob, od;
        own_load(have_row, rw, ox, ob, od, true);
        double sum = 0.0, sum2 = 0.0;
        if (tb >= 0) {
            stage_table(tb);
            if (row < r1) {
                const int pid = A.pat_id[row];
                const int len = plen[pid];
                row_tail(a.x, row, pid * ls, len, 0, sum);
                if (dual_t) row_tail(a.x2, row, pid * ls, len, 0, sum2);
            }
        } else if (!single) {
            // tile without a pattern table: one lane per row straight from val/col
            if (row < r1) {
                for (int j = A.rp[row]; j < A.rp[row + 1]; ++j) {
                    const double vv = A.val[j];
                    const int cc = A.col[j];
                    sum += vv * a.x[cc];
                    if (dual_t) sum2 += vv * a.x2[cc];
                }
            }
        } else {
            // a single long row: the whole workgroup reduces it
            const int s = A.rp[r0], e = A.rp[r1];
            double part = 0.0, part2 = 0.0;
            for (int i = s + tid; i < e; i += kBlock) {
                part += A.val[i] * a.x[A.col[i]];
                if (dual_t) part2 += A.val[i] * a.x2[A.col[i]];
            }
            sum = block_sum(part, red);
            if (dual_t) sum2 = block_sum(part2, red);
        }
        if (have_row) epilogue(rw, sum, sum2, dual_t, ox, ob, od);
    };

    // Per tile the fetches depend on each other (tile bounds -> pattern ids -> x -> y); with
    // NT > 1 each step is issued for NT tiles of the workgroup's sequence before it is waited for.
    for (int t = slot; t < chunk; t += NT * per_xcd) {
        int tile[NT], r0[NT], r1[NT], tb[NT];
        bool together = true;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int tt = t + u * per_xcd;
            tile[u] = tt < chunk ? xcd_tile(A, xcd, tt) : -1;
            r0[u] = r1[u] = 0;
            tb[u] = -1;
            if (tile[u] >= 0) {
                r0[u] = A.tile_row[tile[u]];
                r1[u] = A.tile_row[tile[u] + 1];
                tb[u] = A.tile_table[tile[u]];
            }
            together = together && tile[u] >= 0 && tb[u] >= 0 && tb[u] == tb[0];
        }
        if (!together) {
#pragma unroll
            for (int u = 0; u < NT; ++u)
                if (tile[u] >= 0) one_tile(tile[u], r0[u], r1[u], tb[u]);
            continue;
        }
        stage_table(tb[0]);
        int row[NT], pid[NT];
        bool act[NT], dual_t[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            row[u] = r0[u] + tid;
            act[u] = row[u] < r1[u];
            pid[u] = act[u] ? (int)A.pat_id[row[u]] : 0;
            dual_t[u] = dual && (!A.tile_dual || A.tile_dual[tile[u]]);
        }
        double ox[NT], ob[NT], od[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) own_load(act[u], row[u], ox[u], ob[u], od[u], false);
        int len[NT], base[NT];
        double v[NT][kChunk], xg[NT][kChunk];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            len[u] = act[u] ? plen[pid[u]] : 0;
            base[u] = pid[u] * ls;
            // One gather instruction per entry; the fused dot takes x[row] from the gathers instead
            // of loading it again.  Measured in-box A/B (tools/ab.sh, 256^3, CG iteration time):
            // this kernel -1..-3 % against the unpacked-table version; two tiles per workgroup at a
            // time, an LDS ring of the in-plane x window, and lane shuffles for the near-diagonal
            // entries all land within +-3 %, i.e. inside the drift of one box.
            const int rsafe = act[u] ? row[u] : r0[u];  // idle lanes read a valid address
            bool diag_seen = false;
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                const PatEntry e = ptab[base[u] + k];
                v[u][k] = e.val;
                xg[u][k] = xload(a.x, rsafe, act[u] ? e.off8 : 0);
                if (MODE == kSpmvDot && e.off8 == 0) {
                    ox[u] = xg[u][k];
                    diag_seen = true;
                }
            }
            if (MODE == kSpmvDot && act[u] && !diag_seen) ox[u] = a.x[row[u]];
        }
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            double sum = 0.0, sum2 = 0.0;
#pragma unroll
            for (int k = 0; k < kChunk; ++k)
                if (k < len[u]) sum += v[u][k] * xg[u][k];
            if (len[u] > kChunk) row_tail(a.x, row[u], base[u], len[u], kChunk, sum);
            if (dual_t[u] && act[u]) row_tail(a.x2, row[u], base[u], len[u], 0, sum2);
            if (act[u]) epilogue(row[u], sum, sum2, dual_t[u], ox[u], ob[u], od[u]);
        }
    }
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



int launch_spmv_pattern(const CsrView &A, int mode, const SpmvArgs &a, int grid, hipStream_t s)
{
    const bool wide = A.ncols >= (int64_t(1) << 28);
#define SCHWZ_PAT_LAUNCH(M)                                                                          \
    if (wide)                                                                                        \
        hipLaunchKernelGGL((spmv_pattern_kernel<M, 1, true>), dim3(grid), dim3(kBlock), 0, s, A, a); \
    else                                                                                             \
        hipLaunchKernelGGL((spmv_pattern_kernel<M, 1, false>), dim3(grid), dim3(kBlock), 0, s, A, a);
    switch (mode) {
    case kSpmvPlain: SCHWZ_PAT_LAUNCH(kSpmvPlain) break;
    case kSpmvDot: SCHWZ_PAT_LAUNCH(kSpmvDot) break;
    case kSpmvResidInit: SCHWZ_PAT_LAUNCH(kSpmvResidInit) break;
    case kSpmvResidDual: SCHWZ_PAT_LAUNCH(kSpmvResidDual) break;
    default: SCHWZ_PAT_LAUNCH(kSpmvResidNorm) break;
    }
#undef SCHWZ_PAT_LAUNCH
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

// ---- uploads: the plans of coding_plan.hpp become device arrays bound to CsrView; nothing is decided here ----

// the row-pattern fields of A->v from a plan and the arrays uploaded for it (no arrays: not pattern coded)
static void bind_pattern(schwz_csr *A, const PatternPlan &P)
{
    const auto &b = A->coding.pattern;
    A->v.pat_id = b.pat_id.as<uint8_t>();
    A->v.tile_table = b.tile_table.as<schwz_idx>();
    A->v.tbl_desc = b.tbl_desc.as<schwz_idx>();
    A->v.tbl_len = b.tbl_len.as<uint8_t>();
    A->v.tbl_val = b.tbl_val.as<double>();
    A->v.tbl_delta = b.tbl_delta.as<schwz_idx>();
    A->pattern_fraction = P.fraction;
}

static void bind_dict(schwz_csr *A, const DictPlan &P)
{
    const auto &b = A->coding.dict;
    A->v.code = b.code.as<uint16_t>();
    A->v.vdict_ptr = b.vptr.as<schwz_idx>();
    A->v.ddict_ptr = b.dptr.as<schwz_idx>();
    A->v.vdict = b.vdict.as<double>();
    A->v.ddict = b.ddict.as<schwz_idx>();
    A->dict_fraction = P.fraction;
}

static int upload_pattern(schwz_csr *A, const PatternPlan &P)
{
    auto &b = A->coding.pattern;
    int rc = SCHWZ_OK;
    if (P.built && ((rc = b.pat_id.put(P.pat_id)) || (rc = b.tile_table.put(P.tile_table)) || (rc = b.tbl_desc.put(P.tbl_desc)) ||
                    (rc = b.tbl_len.put(P.tbl_len)) || (rc = b.tbl_val.put(P.tbl_val)) || (rc = b.tbl_delta.put(P.tbl_delta))))
        return rc;
    bind_pattern(A, P);
    return SCHWZ_OK;
}

static int upload_dict(schwz_csr *A, const DictPlan &P)
{
    auto &b = A->coding.dict;
    int rc = SCHWZ_OK;
    if (P.built && ((rc = b.code.put(P.code, 8)) || (rc = b.vptr.put(P.vptr)) || (rc = b.dptr.put(P.dptr)) ||
                    (rc = b.vdict.put(P.vdict)) || (rc = b.ddict.put(P.ddict))))
        return rc;
    bind_dict(A, P);
    return SCHWZ_OK;
}

// what build_spmv_dict releases when an upload fails
static void free_spmv_dict(schwz_csr *A)
{
    A->coding.pattern = {};
    A->coding.dict = {};
    bind_pattern(A, PatternPlan());
    bind_dict(A, DictPlan());
    free_spmv_pair(A);
}

// Row patterns; row pairs and the walk only over accepted patterns (stencil-like matrices); per-entry dictionaries
// only without patterns or when forced.  A coding that is not accepted leaves its fields null and its fraction
// known.  If an upload fails, everything uploaded so far is released and the error returned.
int build_spmv_dict(schwz_csr *A, const schwz_idx *rp, const schwz_idx *col, const double *val,
                    const std::vector<schwz_idx> &tiles)
{
    const CodingOptions opt = coding_options_from_env();
    const HostCsr M{A->v.nrows, A->v.ncols, rp, col, val, tiles};
    int rc;
    {
        StageTimer t("codings: row patterns");
        rc = upload_pattern(A, plan_patterns(opt, M));
    }
    if (!rc && A->v.pat_id) {
        StageTimer t("codings: row pairs + walk tables");
        rc = build_spmv_pair(A, opt, M);
    }
    if (!rc) rc = upload_dict(A, plan_dict(opt, M, A->v.pat_id != nullptr));
    if (rc) free_spmv_dict(A);
    return rc;
}

}  // namespace schwz
