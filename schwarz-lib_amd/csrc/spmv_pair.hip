// Row-PAIR pattern coding of the CSR SpMV: the third, and fastest, lossless coding of this library.
//
// Why.  tools/probes/gather_probe.hip times the bare gather + store structure of a 7-point SpMV at
// 256^3 with no matrix data at all: one row per lane with 8-byte gathers 0.088-0.096 ms, two adjacent
// rows per lane with 16-byte gathers 0.053-0.055 ms.  The row-pattern kernel (spmv_dict.hip, one row
// per lane) sits at 0.115 ms, i.e. on that floor: it is bound by the number of vector-memory
// instructions, not by bytes.  Here a lane owns rows (r, r+1): for an offset d present in either row
// ONE 16-byte load fetches x[r+d] (row r's operand) and x[r+1+d] (row r+1's), halving the gather
// instructions; the matrix costs one byte per PAIR.
//
// Coding.  For a pair, the entries of both rows are merged by offset d = col - row (both rows must
// have strictly ascending columns, so each row still sees its own entries in CSR order); an entry is
// (d, value for row r, value for row r+1, presence bits).  A tile's distinct merged sequences form
// its table (<= 64 patterns, <= 512 entries, staged in LDS); tables are de-duplicated over the
// matrix.  Products are rounded individually and added in the row's entry order: the result is
// bit-identical to the plain CSR kernels.  Tiles that do not qualify run through the plain row code
// of the same launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "coding_plan.hpp"
#include "device_utils.hpp"
#include "schwz_hip.h"
#include "schwz_internal.hpp"

namespace schwz {

// (kPairPats, kPairEntries, kPairChunk, kPairRows, pair_stride: coding_plan.hpp, shared with the plan)
// dynamic shared memory of every launch: values (16 B), offsets (4 B) per staged entry, group masks
constexpr int kPairTableLds = kPairEntries * 16 + kPairEntries * 4 + (kPairEntries / 4) * 4;

struct __attribute__((aligned(16))) PairVal {
    double a, b;
};
struct __attribute__((aligned(8))) PairMeta {
    int off;    // col - row
    int flags;  // bit 0: row r has the entry, bit 1: row r+1 has it
};

typedef double pvd2 __attribute__((ext_vector_type(2)));

// chunk dealt to XCD `xcd` as its j-th one (block-cyclic in runs of 1 << sh), -1 past the end
__device__ __forceinline__ int xcd_chunk(int nchunks, int sh, int xcd, int j)
{
    const int c = ((j >> sh) << (sh + 3)) + (xcd << sh) + (j & ((1 << sh) - 1));
    return c < nchunks ? c : -1;
}

// SINGLE: the whole matrix shares one table (every chunk is coded with table 0): it is staged once
// and no per-chunk lookup precedes the pattern ids.
template <int MODE, bool WIDE, bool SINGLE>
__global__ __launch_bounds__(kBlock) void spmv_pair_kernel(CsrView A, SpmvArgs a)
{
#pragma clang fp contract(off)
    // the staged table lives in dynamic shared memory (kPairTableLds bytes, every launch passes them): the
    // z-sweep walk lays its ring of plane windows over it once the canonical slots have been derived
    extern __shared__ __attribute__((aligned(16))) char pair_lds[];
    PairVal *const pv = reinterpret_cast<PairVal *>(pair_lds);
    int *const poff = reinterpret_cast<int *>(pair_lds + kPairEntries * sizeof(PairVal));  // col - row of the entry
    int *const pmask = poff + kPairEntries;  // per group of CH entries: bit k = row r has entry k, bit 8+k = row r+1
    // gathers issued back to back per lane; the upper-triangle tables of kSpmvDotSym are about half as long
    constexpr bool kDirVec = MODE == kSpmvDirDotSymVec;
    constexpr bool kDir = MODE == kSpmvDirDotSym || kDirVec;
    constexpr bool kSym = MODE == kSpmvDotSym || kDir;
    constexpr int CH = kSym ? kPairChunk / 2 : kPairChunk;
    constexpr bool kDotOnly = MODE == kSpmvDotOnly || kSym;
    __shared__ int plen[kPairPats];            // length | (a gathered entry has col - row == 0) << 16
    __shared__ int pmin[kPairPats], pmax[kPairPats];  // smallest / largest col - row the pattern gathers at
    // canonical stencil layout (CsrView::pair_canon): every pattern expanded to the 7 fixed slots, with
    // presence bits; -1: the pattern has an entry outside the layout
    constexpr bool kCanon = SINGLE && !kSym;
    __shared__ PairVal cpv[kCanon ? kPairPats * 8 : 1];
    __shared__ int cmask[kCanon ? kPairPats : 1];
    const bool canon_on = kCanon && A.pair_canon[7] != 0;
    if (MODE == kSpmvDot || MODE == kSpmvResidInit || kDotOnly) {
        if (a.stop_iter && a.it >= *a.stop_iter) return;
    }
    __shared__ double red[4];
    double cg_alpha = 0.0, cg_beta = 0.0, cg_rho_new = 0.0, cg_rr = 0.0;
    if (kDir) {
        if (a.it >= a.cg_state->stop_iter) return;
        cg_rho_new = fold_partials(a.pq_partials, a.pq_nparts, red);
        cg_rr = fold_partials(a.pq_partials + a.pq_nparts, a.pq_nparts, red);
        cg_beta = cg_rho_new / a.cg_state->rho[a.it & 1];
    }
    if (MODE == kSpmvCgUpdate) {
        if (a.it >= a.cg_state->stop_iter) return;
        cg_alpha = a.cg_state->rho[a.it & 1] / fold_partials(a.pq_partials, a.pq_nparts, red);
        if (a.alpha_out && blockIdx.x == 0 && threadIdx.x == 0) *a.alpha_out = cg_alpha;
    }
    const int tid = threadIdx.x;
    const int xcd = blockIdx.x % kXcds;
    const int slot = blockIdx.x / kXcds;
    const int per_xcd = gridDim.x / kXcds;
    const int nrows = (int)A.nrows;
    const int nchunks = (nrows + kPairRows - 1) / kPairRows;
    const int sh = A.pair_shift;
    const int slots = ((nchunks + (kXcds << sh) - 1) >> (sh + 3)) << sh;  // sequence slots per XCD
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    const bool dual = (MODE == kSpmvResidDual) && a.x2 != nullptr;
    constexpr bool kWantOwn = MODE == kSpmvDot || kDotOnly || MODE == kSpmvCgUpdate;  // x[row] itself
    int cached = -1, ls = 0, tl = 0;  // staged table, its row stride, its longest pattern

    auto stage_table = [&](int tb) {  // workgroup-uniform
        const int td = kSym ? A.pair_sym_base + tb : tb;
        const int eoff = A.ptbl_desc[5 * td], loff = A.ptbl_desc[5 * td + 1];
        const int npat = A.ptbl_desc[5 * td + 2], lmax = A.ptbl_desc[5 * td + 3];
        ls = pair_stride(lmax, CH);
        tl = lmax;
        lds_barrier();  // everyone is done with the previous table
        for (int i = tid; i < npat * ls; i += kBlock) {
            const int pt = i / ls, k = i - pt * ls;
            PairVal v = {0.0, 0.0};
            int off = 0;
            if (k < lmax) {
                const int e = eoff + pt * lmax + k;
                v.a = A.ptbl_val[2 * e];
                v.b = A.ptbl_val[2 * e + 1];
                off = A.ptbl_meta[2 * e];
            }
            pv[i] = v;
            poff[i] = off;
        }
        for (int i = tid; i < npat * ls / CH; i += kBlock) {
            const int pt = i / (ls / CH), k0 = (i - pt * (ls / CH)) * CH;
            int m = 0;
            for (int k = 0; k < CH && k0 + k < lmax; ++k) {
                const int fl = A.ptbl_meta[2 * (eoff + pt * lmax + k0 + k) + 1];
                m |= (fl & 1) << k;
                m |= ((fl >> 1) & 1) << (kPairChunk + k);
            }
            pmask[i] = m;
        }
        lds_barrier();
        if (tid < npat) {
            // does a gather of this pattern (padding included) fetch x[r], x[r + 1] themselves?
            const int len = A.ptbl_len[loff + tid];
            int zero = 0, mn = 0, mx = 0;  // the padding entries gather at offset 0
            // entries at or past the longest pattern of the table are padding for every lane: no
            // launch gathers them
            for (int k = 0; k < min(pair_stride(len, CH), lmax); ++k) {
                const int off = poff[tid * ls + k];
                zero |= off == 0;
                mn = min(mn, off);
                mx = max(mx, off);
            }
            plen[tid] = len | (zero << 16);
            pmin[tid] = mn;
            pmax[tid] = mx;
            if (kCanon && canon_on) {
                // slot of each entry: the first layout slot with its offset (duplicated filler slots
                // therefore never receive one)
                int cm = 0;
                for (int k = 0; k < 8; ++k) cpv[tid * 8 + k] = PairVal{0.0, 0.0};
                const int gm = len ? pmask[(tid * ls) / CH] : 0;
                for (int k = 0; k < len && cm >= 0; ++k) {
                    const int off = poff[tid * ls + k];
                    int slot = -1;
                    for (int q = 6; q >= 0; --q)
                        if (A.pair_canon[q] == off) slot = q;
                    if (slot < 0 || len > CH) {
                        cm = -1;
                        break;
                    }
                    cpv[tid * 8 + slot] = pv[tid * ls + k];
                    cm |= ((gm >> k) & 1) << slot;
                    cm |= ((gm >> (kPairChunk + k)) & 1) << (kPairChunk + slot);
                }
                cmask[tid] = cm;
            }
        }
        lds_barrier();
        cached = tb;
    };
    // x[c], x[c + 1] -- the operands of one merged entry for rows r and r + 1 -- by ONE 16-byte load
    auto ld16 = [&](const double *xv, int c) -> pvd2 {
        pvd2 t;
        if (WIDE) {
            __builtin_memcpy(&t, xv + c, 16);
        } else {
            const uint32_t o = (uint32_t)c * 8u;  // scalar base + 32-bit lane offset
            __builtin_memcpy(&t, reinterpret_cast<const char *>(xv) + o, 16);
        }
        return t;
    };
    // Both rows' dot products with xv.  `safe`: some lane of the wave has a pattern whose 16-byte
    // gathers could leave the vector (first / last column): those waves load each operand that
    // exists on its own.
    auto accumulate = [&](const double *xv, int ra, int base, int len, bool safe, double &s0, double &s1,
                          pvd2 &own, bool want_own) {
        for (int j = 0; j < len; j += CH) {
            const int mask = pmask[(base + j) / CH];
            const bool skip_last = CH == kPairChunk && j + CH - 1 >= tl;  // workgroup-uniform; groups of 8 only
            pvd2 t[CH];
            if (!safe) {
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    // the last slot of a group is padding for every lane when the table's longest
                    // pattern ends one short of it (7 entries in groups of 8: the 7-point stencil):
                    // one straight-line copy of the loads without it (a per-slot test would break
                    // the back-to-back issue of the gathers: measured 0.100 -> 0.141 ms)
                    if (k == CH - 1 && skip_last) continue;
                    const int off = poff[base + j + k];
                    t[k] = ld16(xv, ra + off);
                    if (want_own && off == 0) own = t[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int c = ra + poff[base + j + k];
                    t[k].x = (mask >> k) & 1 ? xv[c] : 0.0;
                    t[k].y = (mask >> (kPairChunk + k)) & 1 ? xv[c + 1] : 0.0;
                }
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const PairVal v = pv[base + j + k];
                if ((mask >> k) & 1) s0 += v.a * t[k].x;
                if ((mask >> (kPairChunk + k)) & 1) s1 += v.b * t[k].y;
            }
        }
    };
    // The same sums for a wave whose patterns all live in the canonical stencil layout: six gathers at
    // workgroup-uniform offsets; the operands of the offset-0 slot, x[r] and x[r + 1], are the second
    // half of the -1 gather and the first half of the +1 gather.  Products in slot order = entry order,
    // absent entries masked: the same bits as the generic walk.
    auto accumulate_canon = [&](const double *xv, int ra, int pid, double &s0, double &s1, pvd2 &own) {
        const int mask = cmask[pid];
        pvd2 t[7];
        t[0] = ld16(xv, ra + A.pair_canon[0]);
        t[1] = ld16(xv, ra + A.pair_canon[1]);
        t[2] = ld16(xv, ra - 1);
        t[4] = ld16(xv, ra + 1);
        t[5] = ld16(xv, ra + A.pair_canon[5]);
        t[6] = ld16(xv, ra + A.pair_canon[6]);
        t[3].x = t[2].y;
        t[3].y = t[4].x;
        own = t[3];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const PairVal v = cpv[pid * 8 + k];
            if ((mask >> k) & 1) s0 += v.a * t[k].x;
            if ((mask >> (kPairChunk + k)) & 1) s1 += v.b * t[k].y;
        }
    };
    // kSpmvDirDotSym: the new search direction p' = z + beta p at column c, z = D^-1 r -- one
    // expression for the stored copy and for every neighbour's recomputed one
    auto dir2 = [&](pvd2 rv, pvd2 pv, pvd2 dv) -> pvd2 {
        const pvd2 z = a.diag_mode ? dv * rv : rv;
        pvd2 o;
        o.x = __builtin_fma(cg_beta, pv.x, z.x);
        o.y = __builtin_fma(cg_beta, pv.y, z.y);
        return o;
    };
    auto dir1 = [&](int c) -> double {
        const double rv = a.cg_r[c];
        const double z = kDirVec ? a.dinv[c] * rv : (a.diag_mode ? a.diag_uniform * rv : rv);
        return __builtin_fma(cg_beta, a.x[c], z);
    };
    auto accumulate_dir = [&](int ra, int base, int len, bool safe, double &s0, double &s1, pvd2 &own) {
        const pvd2 du = {a.diag_uniform, a.diag_uniform};
        for (int j = 0; j < len; j += CH) {
            const int mask = pmask[(base + j) / CH];
            pvd2 t[CH];
            if (!safe) {
                pvd2 tr[CH], tp[CH], td[kDirVec ? CH : 1];
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int off = poff[base + j + k];
                    tr[k] = ld16(a.cg_r, ra + off);
                    tp[k] = ld16(a.x, ra + off);
                    if (kDirVec) td[k] = ld16(a.dinv, ra + off);
                }
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    t[k] = dir2(tr[k], tp[k], kDirVec ? td[kDirVec ? k : 0] : du);
                    if (poff[base + j + k] == 0) own = t[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int c = ra + poff[base + j + k];
                    t[k].x = (mask >> k) & 1 ? dir1(c) : 0.0;
                    t[k].y = (mask >> (kPairChunk + k)) & 1 ? dir1(c + 1) : 0.0;
                }
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const PairVal v = pv[base + j + k];
                if ((mask >> k) & 1) s0 += v.a * t[k].x;
                if ((mask >> (kPairChunk + k)) & 1) s1 += v.b * t[k].y;
            }
        }
    };
    // one row straight from val / col (chunks that are not pair coded)
    auto plain_row = [&](int row, bool dual_t, double &sum, double &sum2) {
        for (int j = A.rp[row]; j < A.rp[row + 1]; ++j) {
            double vv = A.val[j];
            const int cc = A.col[j];
            if (kSym) {  // upper triangle, off-diagonal entries twice
                if (cc < row) continue;
                if (cc > row) vv *= 2.0;
            }
            if (kDir) {
                sum += vv * dir1(cc);
                continue;
            }
            sum += vv * a.x[cc];
            if (dual_t) sum2 += vv * a.x2[cc];
        }
    };
    auto finish = [&](int rw, double sum, double sum2, bool dual_t, double ox, double ob, double od, double &yv,
                      double &pz) {
        yv = sum;
        pz = 0.0;
        if (MODE == kSpmvPlain) {
            yv = (a.beta == 0.0) ? a.alpha * sum : a.alpha * sum + a.beta * ob;
        } else if (MODE == kSpmvDot || kDotOnly) {
            acc0 += ox * sum;
        } else if (MODE == kSpmvCgUpdate) {
            // ob: r_i, od: 1/diag_i, ox: p_i, sum: q_i = (A p)_i; yv <- new r_i; pz <- alpha p_i (x increment)
            const double r = ob - cg_alpha * sum;
            const double z = a.diag_mode ? od * r : r;
            yv = r;
            pz = cg_alpha * ox;
            acc0 += r * z;
            acc1 += r * r;
        } else if (MODE == kSpmvResidInit || MODE == kSpmvResidDual) {
            const double r = ob - sum;
            const double z = (a.dinv || a.diag_mode == 3) ? od * r : r;
            yv = r;
            pz = z;
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

    // run-length record of a chunk's pattern ids (first word 0xffff: none, the ids are bytes per pair).
    // chunk is workgroup-uniform and the table is never written by a kernel: read through the constant
    // address space, i.e. with a scalar load that costs no vector-memory slot
    struct RleRec {
        uint4 lo, hi;  // hi: runs 8-15 of a 16-run record
    };
    const bool rle16 = A.pair_rle_runs == 16;
    auto load_rle = [&](int chunk) -> RleRec {
        RleRec rle = {{0xffffu, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        if (A.pair_rle) {
            typedef const unsigned __attribute__((address_space(4))) *const_words;
            const const_words q = (const_words)(uintptr_t)(A.pair_rle + (rle16 ? 2 * chunk : chunk));
            rle.lo.x = q[0];
            rle.lo.y = q[1];
            rle.lo.z = q[2];
            rle.lo.w = q[3];
            if (rle16) {
                rle.hi.x = q[4];
                rle.hi.y = q[5];
                rle.hi.z = q[6];
                rle.hi.w = q[7];
            }
        }
        return rle;
    };
    // pattern id of the pair starting at row ra: the id of the last run that starts at or before this
    // lane's pair (runs ascending, unused slots repeat the last run)
    auto pid_of = [&](const RleRec rle, int ra) -> int {
        int pid;
        if ((rle.lo.x & 0xffffu) != 0xffffu) {
            const unsigned w[8] = {rle.lo.x, rle.lo.y, rle.lo.z, rle.lo.w, rle.hi.x, rle.hi.y, rle.hi.z, rle.hi.w};
            pid = (int)((w[0] >> 8) & 0xffu);
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                const unsigned e = (w[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
                if ((unsigned)tid >= (e & 0xffu)) pid = (int)(e >> 8);
            }
            if (rle16) {  // workgroup-uniform
#pragma unroll
                for (int k = 8; k < 16; ++k) {
                    const unsigned e = (w[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
                    if ((unsigned)tid >= (e & 0xffu)) pid = (int)(e >> 8);
                }
            }
        } else {
            pid = A.pair_id[ra >> 1];
        }
        return pid;
    };
    auto pair_pid = [&](int chunk, int ra) -> int { return pid_of(load_rle(chunk), ra); };
    // Fixed chunks of 512 consecutive rows, one pair per lane: nothing but the chunk's table id has
    // to be looked up before the pattern ids and the gathers can be requested.
    if (SINGLE) stage_table(0);
    // listed walk: the chunks no z-sweep segment covers (CsrView::sweep_gen), the companion launch of
    // spmv_pair_sweep_kernel below; its partial sums go behind that kernel's (a.part_offset)
    // (kSpmvResidNorm, a.sweep == 2: the chunks of the planes where the fused check residual needs its own
    // product, CsrView::dual_chunks -- the second launch of a dual start in the walk)
    const bool listed = SINGLE && (MODE == kSpmvCgUpdate || MODE == kSpmvDirDotSym || MODE == kSpmvResidNorm) && a.sweep != 0;
    const bool dual_list = MODE == kSpmvResidNorm && a.sweep == 2;
    const int gen_first = listed ? (int)blockIdx.x : slot;
    const int gen_count = listed ? (dual_list ? A.dual_nchunks : A.sweep_ngen) : slots;
    const int gen_stride = listed ? (int)gridDim.x : per_xcd;
    for (int j = gen_first; j < gen_count; j += gen_stride) {
        const int chunk = listed ? (dual_list ? A.dual_chunks[j] : A.sweep_gen[j]) : xcd_chunk(nchunks, sh, xcd, j);
        if (chunk < 0) continue;
        const int tb = SINGLE ? 0 : A.chunk_ptable[chunk];
        const bool dual_t = dual && (!A.chunk_dual || A.chunk_dual[chunk]);
        if (!SINGLE && tb >= 0 && tb != cached) stage_table(tb);
        const int ra = chunk * kPairRows + 2 * tid;
        if (ra >= nrows) continue;
        const bool has_b = ra + 1 < nrows;
        // own operands of the fused epilogues, requested ahead of the gathers
        double ob0 = 0.0, ob1 = 0.0, od0 = 1.0, od1 = 1.0;
        if (MODE == kSpmvResidNorm) {
            if (ra < a.row_limit) ob0 = a.b[ra];
            if (has_b && ra + 1 < a.row_limit) ob1 = a.b[ra + 1];
        }
        if (MODE == kSpmvResidInit || MODE == kSpmvResidDual) {
            // b and 1/diag only stream through: one 16-byte non-temporal load each (the caller's b
            // need not be 16-byte aligned), so that they do not push the gathered x lines out of L2
            typedef double pvd2u __attribute__((ext_vector_type(2), aligned(8)));
            if (has_b) {
                const pvd2u bb = __builtin_nontemporal_load(reinterpret_cast<const pvd2u *>(a.b + ra));
                ob0 = bb.x;
                ob1 = bb.y;
            } else {
                ob0 = a.b[ra];
            }
            if (a.diag_mode == 3) {
                od0 = od1 = a.diag_uniform;
            } else if (a.dinv) {
                if (has_b) {
                    const pvd2u dd = __builtin_nontemporal_load(reinterpret_cast<const pvd2u *>(a.dinv + ra));
                    od0 = dd.x;
                    od1 = dd.y;
                } else {
                    od0 = a.dinv[ra];
                }
            }
        }
        if (MODE == kSpmvPlain && a.beta != 0.0) {
            ob0 = a.y[ra];
            if (has_b) ob1 = a.y[ra + 1];
        }
        pvd2 cgx = {0.0, 0.0};
        if (MODE == kSpmvCgUpdate) {  // r and x of the pair, 1/diag
            if (has_b) {
                // x and r only stream through (read once, written once per launch): non-temporal, so
                // they do not push the gathered p lines out of the XCD's L2 (in-box A/B of the CG
                // iteration: 0.2525 -> 0.2398 ms at 256^3, 0.2632 -> 0.2475 ms on the 512 x 512 x 64 slab,
                // whose +-plane neighbours are 2 MB apart)
                const pvd2 rr = __builtin_nontemporal_load(reinterpret_cast<const pvd2 *>(a.cg_r + ra));
                if (a.cg_x) cgx = __builtin_nontemporal_load(reinterpret_cast<const pvd2 *>(a.cg_x + ra));
                ob0 = rr.x;
                ob1 = rr.y;
            } else {
                ob0 = a.cg_r[ra];
                if (a.cg_x) cgx.x = a.cg_x[ra];
            }
            if (a.diag_mode == 1) {
                if (has_b) {
                    const pvd2 dd = __builtin_nontemporal_load(reinterpret_cast<const pvd2 *>(a.dinv + ra));
                    od0 = dd.x;
                    od1 = dd.y;
                } else {
                    od0 = a.dinv[ra];
                }
            } else if (a.diag_mode == 3) {
                od0 = od1 = a.diag_uniform;
            }
        }
        double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
        pvd2 own = {0.0, 0.0};
        bool own_from_gathers = false;
        if (tb >= 0) {
            const int pid = pair_pid(chunk, ra);
            const int lenz = plen[pid];
            const int len = lenz & 0xffff;
            const int base = pid * ls;
            // a 16-byte gather at offset d reads x[ra + d] and x[ra + d + 1] whether or not both rows have
            // the entry: the lane is an edge lane when that could leave [0, ncols) for ITS pattern (a
            // subdomain's overlap rows sit at the end of the local numbering, so a table-wide bound
            // would send every wave of an interior subdomain down the safe path)
            const bool edge = ra + pmin[pid] < 0 || ra + 1 + pmax[pid] >= (int)A.ncols;
            const bool safe = __builtin_amdgcn_ballot_w64(edge) != 0;
            // the fused dot needs x[ra], x[ra + 1]: the padding entries (col - row = 0) gather exactly
            // that pair, as does a diagonal entry; waves on the safe path load it themselves
            own_from_gathers = kWantOwn && !safe && (lenz >> 16) != 0;
            pvd2 unused = {0.0, 0.0};
            bool canon = false;
            if (kCanon && canon_on) {
                const bool fits = cmask[pid] >= 0 && ra + A.pair_canon[0] >= 0 &&
                                  ra + 1 + A.pair_canon[6] < (int)A.ncols;
                canon = __builtin_amdgcn_ballot_w64(!fits) == 0;
            }
            if (kCanon && canon) {
                accumulate_canon(a.x, ra, pid, s0, s1, own);
                own_from_gathers = kWantOwn;
                if (dual_t) accumulate_canon(a.x2, ra, pid, t0, t1, unused);
            } else if (kDir) {
                accumulate_dir(ra, base, len, safe, s0, s1, own);
            } else {
                accumulate(a.x, ra, base, len, safe, s0, s1, own, own_from_gathers);
                if (dual_t) accumulate(a.x2, ra, base, len, safe, t0, t1, unused, false);
            }
        } else {
            plain_row(ra, dual_t, s0, t0);
            if (has_b) plain_row(ra + 1, dual_t, s1, t1);
        }
        if (kWantOwn && !own_from_gathers) {
            own.x = kDir ? dir1(ra) : a.x[ra];
            if (has_b) own.y = kDir ? dir1(ra + 1) : a.x[ra + 1];
        }
        double y0, y1 = 0.0, p0, p1 = 0.0;
        finish(ra, s0, t0, dual_t, own.x, ob0, od0, y0, p0);
        if (has_b) finish(ra + 1, s1, t1, dual_t, own.y, ob1, od1, y1, p1);
        if (MODE == kSpmvCgUpdate) {
            if (has_b) {
                const pvd2 rr = {y0, y1};
                const pvd2 xx = {cgx.x + p0, cgx.y + p1};
                __builtin_nontemporal_store(rr, reinterpret_cast<pvd2 *>(a.cg_r + ra));
                if (a.cg_x) __builtin_nontemporal_store(xx, reinterpret_cast<pvd2 *>(a.cg_x + ra));
            } else {
                a.cg_r[ra] = y0;
                if (a.cg_x) a.cg_x[ra] = cgx.x + p0;
            }
        } else if (kDir) {  // the pair's own new direction
            if (has_b)
                __builtin_memcpy(a.y + ra, &own, 16);
            else
                a.y[ra] = own.x;
        } else if (MODE != kSpmvResidNorm && !kDotOnly) {
            if (has_b) {
                const pvd2 yy = {y0, y1};
                if (MODE == kSpmvResidInit || MODE == kSpmvResidDual)  // r of the CG start: written once, read much later
                    __builtin_nontemporal_store(yy, reinterpret_cast<pvd2 *>(a.y + ra));
                else
                    __builtin_memcpy(a.y + ra, &yy, 16);
            } else {
                a.y[ra] = y0;
            }
        }
        if (MODE == kSpmvResidInit || MODE == kSpmvResidDual) {
            if (has_b) {
                const pvd2 pp = {p0, p1};
                __builtin_nontemporal_store(pp, reinterpret_cast<pvd2 *>(a.p + ra));
            } else {
                a.p[ra] = p0;
            }
        }
    }
    if (MODE != kSpmvPlain) {
        const double s0 = block_sum(acc0, red);
        const double s1 = block_sum(acc1, red);
        if (tid == 0) {
            const int stride = a.part_stride ? a.part_stride : (int)gridDim.x;
            a.partials[a.part_offset + blockIdx.x] = s0;
            a.partials[stride + a.part_offset + blockIdx.x] = s1;
        }
        if (MODE == kSpmvResidDual) {
            const double s2v = block_sum(acc2, red);
            if (tid == 0) a.partials[2 * gridDim.x + blockIdx.x] = s2v;
        }
    }
    if (kDir && blockIdx.x == 0 && tid == 0 && !a.sweep) {  // (the z-sweep kernel does it for its companion launch)
        // what cg_direction_kernel's workgroup 0 does
        cg_advance_state(const_cast<CgState *>(a.cg_state), a.it, cg_rho_new, cg_rr, a.cg_rtol);
    }
}

// The z-sweep walks below have one form each.  The alternatives they were measured against (masked sums, plain or
// hinted streams, the earlier prologues, the two-slot halo ring) were build-time switches until commit 1043a3a;
// DESIGN.md section 3 and profiles/ keep the measurements.
//
// Sums.  The slot tables hold a coefficient of +0.0 wherever a pattern has no entry (CsrView::canon_ready, made once by
// the plan) and the walks sum EVERY slot's product instead of selecting +0.0 for the absent ones by a mask bit (two bit
// tests and two 64-bit selects per slot and row pair: a third of the vector instructions of a step).  The same bits: a
// sum that began at +0.0 is never -0.0, so adding the +-0.0 that (+0.0 x a finite operand) yields leaves it unchanged,
// exactly like adding a selected +0.0.  The operands of absent slots are loaded vector data (clamped addresses, windows
// of real planes), finite whenever the vector is; a vector holding Inf / NaN has a NaN p.(A p) either way.
//
// Streams.  The update walk's r is a non-temporal load and store and p' leaves the fused launch with non-temporal stores.
// On vectors of 135 MB (256^3, 512 x 512 x 64) the hints win: in-box a plain r load in the update launch costs the
// FOLLOWING fused launch 4 us of 74, a plain r store the update launch 3 us of 69.  Where r, p and p' fit the 256 MiB
// Infinity Cache together (192^3: 3 x 57 MB) they LOSE 5 % of the step -- they give up the on-die copy the next launch
// would have read (profiles/r03_cache_hints.txt).  A per-launch choice was built and dropped: as a workgroup-uniform
// branch around the three accesses it cost 2.5 % of the 256^3 step (the loop body is no longer one block), as a template
// parameter it doubles ~100 instantiations; no configuration of BASELINE.json has vectors that small.
// r0 leaves the START walk with a plain store: its next two readers (first direction, first update) follow at once and
// find part of it on die: -0.5 ... -0.75 % per step at 256^3 / 512 x 512 x 64, neutral on 1 GB vectors (same file).
//
// Prologue: what a walk workgroup does before its first step -- a constant per launch that does not depend on the bytes
// (profiles/r16_walk_timeline.txt, r21_walk_prologue.txt).  Two steps:
// 1. Everything that depends on nothing but the kernel arguments and blockIdx.x is requested at kernel entry before
//    anything is waited for -- stop_iter, rho, the slot's WalkRecord (segment AND its first five chain rows, read through
//    the constant address space: scalar loads that do not queue behind the vector loads), the table entries in their
//    staged form (one unconditional 16-byte load per entry, kept in registers) and the lane's strided sums of the
//    previous launch's partial sums, eight per bank at a time (fold_lane_sums) -- and the early return and the
//    empty-slot branch follow that one wait.  The loads in front of the return have no side effect and valid addresses
//    whether or not the launch is live.
// 2. Then the windows are requested, and BEHIND those requests the tables go to LDS and the cross-wave part of the fold
//    gives alpha / beta, behind barriers that order LDS alone (block_sum_lds; the fused direction walk's two folds
//    share them).  Requested behind the windows, tables and partial sums came back behind them (vector loads return in
//    order), and a fold's __syncthreads() waited for every prefetched plane, not only for those of the first position.
// Every sum keeps its order: the same bits as folding one partial sum after the other.

// table entries a lane keeps in registers between kernel entry and the LDS stores: kPairPats patterns of nine slots at
// the most, of five in the fused direction walk
constexpr int kWalkTabPerLane = (kPairPats * 9 + kBlock - 1) / kBlock;
constexpr int kWalkSymTabPerLane = (kPairPats * 5 + kBlock - 1) / kBlock;

// Launch timeline of the walk kernels (measurement build only: make variant DEFS=-DSCHWZ_WITH_PROBES, read by
// tools/walk_timeline.py).  Lane 0 of a workgroup stores the 100 MHz wall clock at kWalkStamps points of its life into
// SpmvArgs::walk_probe: [form | blockIdx << 8 | XCC id << 40, chain positions of the segment, stamps...].  In the
// product SCHWZ_STAMP is empty.
// SCHWZ_WALK_STAMP_WAIT=1: the "windows" stamp first waits for every load in flight, i.e. it says when the first
// windows have landed, not when they were requested (this changes what is measured behind it).
enum { kStampEntry, kStampSegment, kStampWindows, kStampTables, kStampFirstStep, kStampLastStep, kStampDone, kWalkStamps };
enum { kFormUpdate = 1, kFormStart = 2, kFormDirdot = 3, kFormFirst = 4 };
#ifdef SCHWZ_WITH_PROBES
constexpr int kWalkStampWords = 2 + kWalkStamps;
#ifndef SCHWZ_WALK_STAMP_WAIT
#define SCHWZ_WALK_STAMP_WAIT 0
#endif
__device__ __forceinline__ void walk_stamp(const SpmvArgs &a, int form, int k)
{
    if (threadIdx.x == 0 && a.walk_probe) {
        unsigned long long *rec = a.walk_probe + (size_t)blockIdx.x * kWalkStampWords;
        if (k == kStampEntry) {
            const unsigned long long xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11)) & 0xfu;  // HW_REG_XCC_ID, bits 3:0
            rec[0] = (unsigned long long)form | ((unsigned long long)blockIdx.x << 8) | (xcc << 40);
        }
        rec[2 + k] = wall_clock64();
    }
}
__device__ __forceinline__ void walk_stamp_positions(const SpmvArgs &a, int npos)
{
    if (threadIdx.x == 0 && a.walk_probe) a.walk_probe[(size_t)blockIdx.x * kWalkStampWords + 1] = (unsigned long long)npos;
}
#define SCHWZ_STAMP(form, k) walk_stamp(a, form, k)
// a scalar the stamp behind it has to wait for (the chain rows: scalar loads)
#define SCHWZ_STAMP_AFTER(value) asm volatile("" ::"s"(value))
#define SCHWZ_STAMP_POSITIONS(npos) walk_stamp_positions(a, npos)
#define SCHWZ_STAMP_LANDED()                                           \
    do {                                                               \
        if (SCHWZ_WALK_STAMP_WAIT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    } while (0)
#else
#define SCHWZ_STAMP(form, k) ((void)0)
#define SCHWZ_STAMP_AFTER(value) ((void)0)
#define SCHWZ_STAMP_POSITIONS(npos) ((void)0)
#define SCHWZ_STAMP_LANDED() ((void)0)
#endif

// Workgroup 0 of a walk zeroes the partial-sum slots no workgroup of the launch or of its companion writes, in
// BANKS banks of a.part_stride slots
template <int BANKS>
__device__ __forceinline__ void zero_unused_partials(const SpmvArgs &a)
{
    if (blockIdx.x == 0)
        for (int i = (int)gridDim.x + a.part_offset + (int)threadIdx.x; i < a.part_stride; i += kBlock) {
            a.partials[i] = a.partials[a.part_stride + i] = 0.0;
            if (BANKS == 3) a.partials[2 * a.part_stride + i] = 0.0;
        }
}

// Row of a 16-byte piece clamped into the vector: pieces beyond its ends (first / last band of a plane) read a valid
// address; no row has an entry there and the zero coefficients drop what they deliver
__device__ __forceinline__ int clamp_piece(int g, int64_t gmax) { return g < 0 ? 0 : (g > (int)gmax ? (int)gmax : g); }

// Window a far slot reads at a chain position, from its two bits of chain_far: 1 the previous position's, 2 the
// next one's, 0 none -- the slot then reads the position's own window, and its coefficients are zero
__device__ __forceinline__ const double *far_window(int sel, const double *prv, const double *nxt, const double *cur)
{
    return (sel & 3) == 1 ? prv : ((sel & 3) == 2 ? nxt : cur);
}

// ---------------------------------------------------------------------------------------------------
// z-sweep ("brick") walk of the q-free CG update launch for matrices in the canonical 3-D stencil layout
// {-PL, -NX, -1, 0, +1, +NX, +PL} (CsrView::sweep_*).  tools/probes/brick_probe.hip priced the memory
// structure first: with six 16-byte gathers per row pair the launch is bound by vector-memory
// instructions and, on wide planes, re-fetches the +-PL lines the 4 MiB L2s cannot hold; here a
// workgroup takes a band of T rows through the planes z0 <= z < z1, fetches each plane's window
// [band - NX, band + T + NX) of p ONCE with coalesced 16-byte loads two planes ahead of its use, and
// reads all seven operands of a row pair from an LDS ring of four windows.  r (and 1/diag) of the
// lane's pairs and the chunk's pattern-id record are requested one plane ahead.  The loop body is
// straight-line code (addresses are clamped instead of guarded, every count is a template
// parameter), so the compiler can give each wait its own vmcnt instead of draining the queue.
// Products and their order are those of accumulate_canon: the same bits per row.
// NL: 16-byte pieces of a window per lane; NH: chunks of 512 rows per band; DIAGVEC: Jacobi diagonal
// as a full vector.  x is not touched (deferred x update only).
// INIT: the same walk as the CG start launch (kSpmvResidInit without its p store): the ring holds the
// windows of the start vector y, r = b - A y is stored to a.y, partial r.z and r.r -- p = D^-1 r is left
// to the first fused direction launch (spmv_pair_dirdot_sweep_kernel<.., FIRST>), which reads r anyway.
// ---------------------------------------------------------------------------------------------------
// DUAL (with INIT): third partial bank = sum of r_i^2 over the chain positions NOT flagged in chain_dual -- the
// part of the fused check residual ||b - A x2||^2 that coincides with the start residual; the flagged planes
// are added by a listed kSpmvResidNorm launch on x2 (launch_spmv_pair).
// RUNS: runs per chunk record of the pattern ids (8: 16 bytes, 16: 32 bytes; CsrView::pair_rle_runs); 0: planes that
// are not whole 512-row chunks (PL % 512 != 0, round 3): the bands of a plane no longer coincide with the chunks
// the records describe, so a lane reads its pair's pattern id as a byte (one coalesced load per 512 rows, requested
// a plane ahead like the record), and the last band of a plane is partial: its lanes beyond the plane's end repeat
// the band's last pair -- same loads, same value stored to the same address -- and add nothing to the sums.
// (The three-positions-ahead halo schedule that pays in the fused direction launch below was measured here too,
// with a third halo slot: no gain on 256- and 512-wide planes, where the p halo already hits L2 -- r is a
// non-temporal stream in this launch and does not evict it --, and a loss wherever the larger ring costs a
// workgroup per CU: profiles/r03_h3_rle16_ab.txt.  Not kept.)
template <int NHL, int NH, bool DIAGVEC, bool INIT = false, bool DUAL = false, int RUNS = 8>
__global__ __launch_bounds__(kBlock) void spmv_pair_sweep_kernel(CsrView A, SpmvArgs a)
{
#pragma clang fp contract(off)
    // dynamic LDS: own parts of four chain positions [4][T], the +-NX halos of two [2][2 NX] (only the plane
    // being computed needs its halo, which is why it is requested one position ahead, not two: its lines are
    // the own lines of the neighbouring bands, i.e. L2 hits), the slot tables of the matrix
    extern __shared__ __attribute__((aligned(16))) char sweep_lds[];
    constexpr int T = NH * kPairRows;
    const int NX = A.sweep_nx;
    double *const own_ring = reinterpret_cast<double *>(sweep_lds);
    double *const halo_ring = own_ring + 4 * T;
    PairVal *const cpv = reinterpret_cast<PairVal *>(halo_ring + 4 * NX);
    const int ntab = A.canon_npat * 9;  // entries of the slot tables
    __shared__ double red[4];
    double cg_alpha = 1.0;
    const int tid = threadIdx.x;
    [[maybe_unused]] constexpr int kForm = INIT ? kFormStart : kFormUpdate;
    SCHWZ_STAMP(kForm, kStampEntry);
    // INIT reads the right-hand side where the update launch reads r (the caller's b need only be 8-byte
    // aligned) and stores r to a.y
    typedef double pvd2u __attribute__((ext_vector_type(2), aligned(8)));
    const double *const r_in = INIT ? a.b : a.cg_r;
    double *const r_out = INIT ? a.y : (a.cg_r_out ? a.cg_r_out : a.cg_r);
    const pvd2 ring_scale = {a.ring_scale, a.ring_scale};  // 1.0 except in the first update of a solve with a virtual p0
    double fold_lane = 0.0, rho_it = 0.0;
    // the lane's table entries between their request and their LDS stores: rounds of kBlock entries, a round that
    // exists is loaded by every lane (the lanes past the table's end repeat its last entry and store nothing)
    pvd2 tab[kWalkTabPerLane];
    auto request_tables = [&]() {
#pragma unroll
        for (int k = 0; k < kWalkTabPerLane; ++k) {
            tab[k] = pvd2{0.0, 0.0};
            if (k * kBlock < ntab) tab[k] = *reinterpret_cast<const pvd2 *>(A.canon_ready + 2 * min(tid + k * kBlock, ntab - 1));
        }
    };
    auto store_tables = [&]() {
#pragma unroll
        for (int k = 0; k < kWalkTabPerLane; ++k)
            if (tid + k * kBlock < ntab) cpv[tid + k * kBlock] = PairVal{tab[k].x, tab[k].y};
    };
    // Prologue, step 1: request everything that depends only on the arguments and blockIdx.x -- stop_iter, rho and the
    // record (scalar), the ready tables, the lane sums -- in front of the first wait
    int stop_iter = 0;
    if (!INIT) {
        stop_iter = a.cg_state->stop_iter;
        rho_it = a.cg_state->rho[a.it & 1];
    }
    // the slot's record -- the segment and the planes of its chain positions z0 - 1 .. z0 + 3 -- through the constant
    // address space: scalar loads
    typedef const WalkRecord __attribute__((address_space(4))) *const_record;
    int4 sg;
    int rec_plane[5] = {0, 0, 0, 0, 0};
    auto request_record = [&]() {
        const const_record rec = (const_record)(uintptr_t)A.sweep_rec + blockIdx.x;
        sg.x = rec->band, sg.y = rec->z0, sg.z = rec->z1, sg.w = rec->rows;
#pragma unroll
        for (int k = 0; k < 5; ++k) rec_plane[k] = rec->plane[k];
    };
    request_record();
    // (no instruction: keeps the compiler from moving the scalar requests above behind the vector requests below, where
    // they landed behind a second wait for kernel arguments -- the arguments those need are operands here, so they
    // arrive with the first batch)
    asm volatile("" ::"s"(a.pq_partials), "s"(a.pq_nparts), "s"(A.canon_ready), "s"(ntab) : "memory");
    request_tables();  // (before the sums: the first wait for a vector load is inside fold_lane_sums)
    if (!INIT) {
        double s[1] = {0.0};
        fold_lane_sums(a.pq_partials, a.pq_nparts, s);
        fold_lane = s[0];
    }
    if (!INIT && a.it >= stop_iter) return;
    // Prologue, step 2, called behind the window requests so that the two latencies overlap instead of adding up at the
    // start of every workgroup's life: tables to LDS, cross-wave fold, alpha (every workgroup folds the partial sums of
    // the previous launch itself)
    auto tables_and_alpha = [&]() {
        store_tables();
        if (!INIT) {
            double v[1] = {fold_lane};
            block_sum_lds(v, red);
            cg_alpha = rho_it / v[0];
            if (blockIdx.x == 0 && tid == 0 && a.alpha_out) *a.alpha_out = cg_alpha;
        }
        lds_barrier();
    };
    zero_unused_partials<DUAL ? 3 : 2>(a);
    const int64_t PL = A.sweep_pl;
    const int band = sg.x, z0 = sg.y, z1 = sg.z;  // chain positions z0 <= z < z1
    constexpr bool GEN = RUNS == 0;
    const int blen = GEN ? sg.w : T;               // rows of the band inside the plane (even)
    const int64_t gmax = A.ncols - 2;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    typedef const unsigned __attribute__((address_space(4))) *const_words;
    typedef const int __attribute__((address_space(4))) *const_ints;
    if (z0 < z1) {
        // first row of the band at a chain position (scalar loads: the position is workgroup-uniform); a
        // position without a plane (the ends of a chain) reads plane 0 -- valid memory whose slots have zero coefficients
        const const_ints chain = (const_ints)(uintptr_t)A.chain_plane;
        const const_ints chain_far = (const_ints)(uintptr_t)A.chain_far;
        auto band_row = [&](int z) -> int {  // rows fit 32 bits (the launch is for ncols < 2^28)
            const int k = chain[z];
            return (k < 0 ? 0 : k) * (int)PL + band * T;
        };
        auto clampg = [&](int g) -> int { return clamp_piece(g, gmax); };
        auto load_own = [&](int base, pvd2 (&reg)[NH]) {
#pragma unroll
            for (int k = 0; k < NH; ++k) __builtin_memcpy(&reg[k], a.x + clampg(base + 2 * (tid + k * kBlock)), 16);
        };
        auto store_own = [&](int z, const pvd2 (&reg)[NH]) {
            double *slot_p = own_ring + (size_t)(z & 3) * T;
#pragma unroll
            for (int k = 0; k < NH; ++k) *reinterpret_cast<pvd2 *>(slot_p + 2 * (tid + k * kBlock)) = ring_scale * reg[k];
        };
        // halo of a plane: the NX rows below the band (pieces 0 .. NX/2) and the NX rows above it
        auto load_halo = [&](int base, pvd2 (&reg)[NHL]) {
            const int lo = base - NX, up = base + T;
#pragma unroll
            for (int k = 0; k < NHL; ++k) {
                const int pc = min(tid + k * kBlock, NX - 1);  // NX pieces: NX/2 below, NX/2 above
                const int g = pc < NX / 2 ? lo + 2 * pc : up + 2 * (pc - NX / 2);
                __builtin_memcpy(&reg[k], a.x + clampg(g), 16);
            }
        };
        auto store_halo = [&](int z, const pvd2 (&reg)[NHL]) {
            double *slot_p = halo_ring + (size_t)(z & 1) * 2 * NX;
#pragma unroll
            for (int k = 0; k < NHL; ++k) {
                const int pc = min(tid + k * kBlock, NX - 1);
                *reinterpret_cast<pvd2 *>(slot_p + 2 * pc) = ring_scale * reg[k];
            }
        };
        struct Ahead {
            pvd2 r, d;
            unsigned w[GEN ? 1 : RUNS / 2];
        };
        auto fetch = [&](int base, int h) -> Ahead {
            Ahead f;
            const int row0 = base + h * kPairRows;
            const int ra = GEN ? base + min(h * kPairRows + 2 * tid, blen - 2) : row0 + 2 * tid;
            if (GEN) {
                f.w[0] = A.pair_id[ra >> 1];
            } else {
                const const_words q = (const_words)(uintptr_t)(A.pair_rle + (row0 / kPairRows) * ((RUNS ? RUNS : 8) / 8));
#pragma unroll
                for (int k = 0; k < (GEN ? 1 : RUNS / 2); ++k) f.w[k] = q[k];
            }
            f.r = __builtin_nontemporal_load(reinterpret_cast<const pvd2u *>(r_in + ra));
            if (DIAGVEC) f.d = __builtin_nontemporal_load(reinterpret_cast<const pvd2 *>(a.dinv + ra));
            return f;
        };
        // Software pipeline, two steps deep, without register copies (the loop is unrolled by two and the
        // register sets alternate): own(z + 3) is requested while position z is computed, into the set whose
        // content -- own(z + 1) -- has just gone to LDS; r(z + 2) at the end of step z, into the set step z
        // has just consumed; the halo of position z + 1 (L2 hits) first thing in step z.  The band's first
        // rows at the positions z - 1 .. z + 3 travel in scalar registers (brow), one new one per step.
        pvd2 own_a[NH], own_b[NH], hreg[NHL];
        Ahead r_a[NH], r_b[NH];
        int brow[5];
#pragma unroll
        for (int k = 0; k < 5; ++k)
            brow[k] = (rec_plane[k] < 0 ? 0 : rec_plane[k]) * (int)PL + band * T;  // band_row(z0 - 1 + k), from the record
        SCHWZ_STAMP_AFTER(brow[0] + brow[1] + brow[2] + brow[3] + brow[4]);
        SCHWZ_STAMP(kForm, kStampSegment);
        SCHWZ_STAMP_POSITIONS(z1 - z0);
        {
            // everything the first two positions need is requested before anything is waited for
            pvd2 first[NH], second[NH];
            load_own(brow[0], first);
            load_own(brow[1], second);
            load_halo(brow[1], hreg);
            load_own(brow[2], own_b);
            load_own(brow[3], own_a);
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                r_a[h] = fetch(brow[1], h);
                r_b[h] = fetch(z0 + 1 < z1 ? brow[2] : brow[1], h);
            }
            SCHWZ_STAMP_LANDED();
            SCHWZ_STAMP(kForm, kStampWindows);
            tables_and_alpha();
            SCHWZ_STAMP(kForm, kStampTables);
            store_own(z0 - 1, first);
            store_own(z0, second);
        }
        // one position: `own_next` holds own(z + 1) on entry and own(z + 3) on exit, `rr` r(z) / r(z + 2)
        auto step = [&](int z, pvd2 (&own_next)[NH], Ahead (&rr)[NH]) {
            // brow[] = first rows at z - 1, z, z + 1, z + 2, z + 3
            store_own(z + 1, own_next);
            store_halo(z, hreg);
            lds_barrier();
            load_halo(brow[2], hreg);
            load_own(brow[4], own_next);
            const int far = chain_far[z];
            const bool plain_pos = DUAL ? ((const_ints)(uintptr_t)A.chain_dual)[z] == 0 : true;
            const double *cur = own_ring + (size_t)(z & 3) * T;
            const double *prv = own_ring + (size_t)((z + 3) & 3) * T;
            const double *nxt = own_ring + (size_t)((z + 1) & 3) * T;
            const double *hlo = halo_ring + (size_t)(z & 1) * 2 * NX, *hup = hlo + NX;
            const double *fb0 = far_window(far, prv, nxt, cur), *fb1 = far_window(far >> 2, prv, nxt, cur);
            const double *fa0 = far_window(far >> 4, prv, nxt, cur), *fa1 = far_window(far >> 6, prv, nxt, cur);
            const int rbase = z + 2 < z1 ? brow[3] : brow[1];  // past the segment: a valid plane, never used
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const Ahead f = rr[h];
                const int i0u = h * kPairRows + 2 * tid;  // position inside the band
                const bool valid = !GEN || i0u < blen;
                const int i0 = GEN ? min(i0u, blen - 2) : i0u;
                const int ra = brow[1] + i0;
                // the id of the last run that starts at or before this lane's pair
                int pid = GEN ? (int)f.w[0] : (int)((f.w[0] >> 8) & 0xffu);
#pragma unroll
                for (int k = 1; k < RUNS; ++k) {
                    const unsigned e = (f.w[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
                    if ((unsigned)tid >= (e & 0xffu)) pid = (int)(e >> 8);
                }
                pvd2 t[8];
                t[4] = *reinterpret_cast<const pvd2 *>(cur + i0);
                t[3].x = i0 > 0 ? cur[i0 - 1] : hlo[NX - 1];
                t[3].y = t[4].x;
                t[5].x = t[4].y;
                t[5].y = i0 + 2 < T ? cur[i0 + 2] : hup[0];
                t[2] = *reinterpret_cast<const pvd2 *>(i0 >= NX ? cur + (i0 - NX) : hlo + i0);
                t[6] = *reinterpret_cast<const pvd2 *>(i0 + NX < T ? cur + (i0 + NX) : hup + (i0 + NX - T));
                t[0] = *reinterpret_cast<const pvd2 *>(fb0 + i0);
                t[7] = *reinterpret_cast<const pvd2 *>(fa0 + i0);
                // sums without branches or selects: an absent entry has a coefficient of +0.0 (see "Sums" above).
                // The second far slots exist on a subdomain's boundary planes only: a plane without them skips both
                // (workgroup-uniform).
                double s0 = 0.0, s1 = 0.0;
                auto add = [&](int k, pvd2 tv) {
                    const PairVal v = cpv[pid * 9 + k];
                    const double p0 = v.a * tv.x, p1 = v.b * tv.y;
                    s0 += p0;
                    s1 += p1;
                };
                add(0, t[0]);
                if (far & 0x0c) add(1, *reinterpret_cast<const pvd2 *>(fb1 + i0));
#pragma unroll
                for (int k = 2; k < 8; ++k) add(k, t[k]);
                if (far & 0xc0) add(8, *reinterpret_cast<const pvd2 *>(fa1 + i0));
                // r -= alpha q ; z = D^-1 r ; partial r.z and r.r  (kSpmvCgUpdate's epilogue, x deferred)
                const double r0 = INIT ? f.r.x - s0 : f.r.x - cg_alpha * s0;
                const double zz0 = a.diag_mode ? (DIAGVEC ? f.d.x : a.diag_uniform) * r0 : r0;
                const double r1 = INIT ? f.r.y - s1 : f.r.y - cg_alpha * s1;
                const double zz1 = a.diag_mode ? (DIAGVEC ? f.d.y : a.diag_uniform) * r1 : r1;
                if (GEN) {
                    const double t00 = r0 * zz0, t01 = r0 * r0, t10 = r1 * zz1, t11 = r1 * r1;
                    acc0 += valid ? t00 : 0.0;
                    acc1 += valid ? t01 : 0.0;
                    acc0 += valid ? t10 : 0.0;
                    acc1 += valid ? t11 : 0.0;
                } else {
                    acc0 += r0 * zz0;
                    acc1 += r0 * r0;
                    acc0 += r1 * zz1;
                    acc1 += r1 * r1;
                }
                if (DUAL) {
                    const double q0 = r0 * r0, q1 = r1 * r1;
                    acc2 += plain_pos ? q0 : 0.0;
                    acc2 += plain_pos ? q1 : 0.0;
                }
                const pvd2 rn = {r0, r1};
                if (INIT)  // r0: a plain store, its readers follow at once ("Streams" above)
                    *reinterpret_cast<pvd2 *>(r_out + ra) = rn;
                else
                    __builtin_nontemporal_store(rn, reinterpret_cast<pvd2 *>(r_out + ra));
                rr[h] = fetch(rbase, h);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) brow[k] = brow[k + 1];
            brow[4] = band_row(z + 4);
            if (z == z0) SCHWZ_STAMP(kForm, kStampFirstStep);
        };
        int z = z0;
        for (; z + 1 < z1; z += 2) {
            step(z, own_b, r_a);
            step(z + 1, own_a, r_b);
        }
        if (z < z1) step(z, own_b, r_a);
        SCHWZ_STAMP(kForm, kStampLastStep);
    } else if (!INIT && blockIdx.x == 0) {
        tables_and_alpha();  // (an empty first slot still reports alpha)
    }
    // (one reduction of all the sums behind a single pair of LDS-only barriers was measured here: inside the noise,
    // profiles/r16_walk_launch_constant.txt.  Not kept.)
    const double s0 = block_sum(acc0, red);
    const double s1 = block_sum(acc1, red);
    if (tid == 0) {
        a.partials[blockIdx.x] = s0;
        a.partials[a.part_stride + blockIdx.x] = s1;
    }
    if (DUAL) {
        const double s2 = block_sum(acc2, red);
        if (tid == 0) a.partials[2 * a.part_stride + blockIdx.x] = s2;
    }
    SCHWZ_STAMP(kForm, kStampDone);
}

// ---------------------------------------------------------------------------------------------------
// The same walk for the fused direction update + p.(A p) launch of symmetric matrices (kSpmvDirDotSym):
// beta from the folded partials, p' = z + beta p (z = D^-1 r, uniform or no Jacobi scaling) computed ONCE
// per element from coalesced loads of r and p -- into the LDS ring, and into the output buffer for the
// positions of the segment -- and the upper-triangle sum p'.(A p') = sum_i p'_i (a_ii p'_i + 2 sum_{j>i}
// a_ij p'_j) read from LDS: slots [0, +1, +NX, far after 0, far after 1].  The chunk-by-chunk form of this
// launch gathers r AND p at every entry; here every element of r and p is loaded once (plus the NX-row
// halo, L2 hits).  Same expression for p' everywhere, same products in the same order: the same bits per
// row.  Workgroup 0 advances CgState like cg_direction_kernel.  NHL / NH as above.
// FIRST: the first direction of a solve whose start launch was the INIT walk above: p' = z (nothing is
// read from p, beta does not exist yet), the partial sums of p'.(A p'), CgState untouched.
// ---------------------------------------------------------------------------------------------------
// Halo schedule and streams (profiles/r03_dd_ab.txt).  The halo of a position is requested THREE positions ahead, i.e.
// in the same step in which the neighbouring band requests the same lines as its own window (hence the third halo slot
// in LDS, kDirdotHaloLines); the own r lines are plain loads (they are the neighbouring band's halo: a non-temporal
// load marks them for early eviction); p' leaves with non-temporal stores.  Asked for two steps after the neighbour had
// fetched the lines -- longer than a line lives in the 4 MiB L2 at this stream rate -- the halo was fetched twice: the
// PMC traffic of the launch was 1.17 x (256-wide planes) / 1.25 x (512-wide) its bytes.  All three together, in-box:
// launch 0.0789 -> 0.0740 ms on the cube, 0.0861 -> 0.0729 ms on the 512 x 512 x 64 slab (0.585 -> 0.69 of peak; the
// step 1.95 -> 1.82 ms), the same bits.
template <int NHL, int NH, bool FIRST = false, int RUNS = 8>
__global__ __launch_bounds__(kBlock) void spmv_pair_dirdot_sweep_kernel(CsrView A, SpmvArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char sweep_lds[];
    constexpr int T = NH * kPairRows;
    const int NX = A.sweep_nx;
    double *const own_ring = reinterpret_cast<double *>(sweep_lds);  // p' of four chain positions [4][T]
    double *const halo_ring = own_ring + 4 * T;                       // p' of the NX rows above the band [kDirdotHaloLines][NX]
    PairVal *const cpv = reinterpret_cast<PairVal *>(halo_ring + kDirdotHaloLines * NX);
    const int ntab = A.canon_npat * 5;  // entries of the slot tables
    __shared__ double red[8];
    [[maybe_unused]] constexpr int kForm = FIRST ? kFormFirst : kFormDirdot;
    SCHWZ_STAMP(kForm, kStampEntry);
    double cg_rho_new = 0.0, cg_rr = 0.0, cg_beta = 0.0;
    const int tid = threadIdx.x;
    // FIRST, workgroup 0: CgState and the check norm from the start walk's partial sums, which the kernel boundary
    // behind that walk made visible (cg_init_finalize_kernel's work; nobody in this launch reads the state)
    auto init_fold = [&]() {
        if (FIRST && a.init_fold && blockIdx.x == 0)
            cg_init_state(const_cast<CgState *>(a.cg_state), a.pq_partials, a.pq_nparts, a.cg_rtol, a.norm_sq_out,
                          a.norm_bank, red);
    };
    double fold_rho = 0.0, fold_rr = 0.0, rho_it = 0.0;
    // the lane's table entries between their request and their LDS stores (as in the update walk)
    pvd2 tab[kWalkSymTabPerLane];
    auto request_tables = [&]() {
#pragma unroll
        for (int k = 0; k < kWalkSymTabPerLane; ++k) {
            tab[k] = pvd2{0.0, 0.0};
            if (k * kBlock < ntab) tab[k] = *reinterpret_cast<const pvd2 *>(A.canon_sym_ready + 2 * min(tid + k * kBlock, ntab - 1));
        }
    };
    auto store_tables = [&]() {
#pragma unroll
        for (int k = 0; k < kWalkSymTabPerLane; ++k)
            if (tid + k * kBlock < ntab) cpv[tid + k * kBlock] = PairVal{tab[k].x, tab[k].y};
    };
    // Prologue, step 1 (as in the update walk): requests only, in front of the first wait.
    // (FIRST reads nothing of CgState: with init_fold its own workgroup 0 is still to write it.  After a zero start
    // residual the launch is needless; the update launch behind it sees stop_iter == 0 and leaves.)
    int stop_iter = 0;
    if (!FIRST) {
        stop_iter = a.cg_state->stop_iter;
        rho_it = a.cg_state->rho[a.it & 1];
    }
    // the slot's record -- the segment and the planes of its chain positions z0 - 1 .. z0 + 3 -- through the constant
    // address space: scalar loads (of its own table: the band height may differ from the update launch's)
    typedef const WalkRecord __attribute__((address_space(4))) *const_record;
    int4 sg;
    int rec_plane[5] = {0, 0, 0, 0, 0};
    auto request_record = [&]() {
        const const_record rec = (const_record)(uintptr_t)A.sweep_rec_dir + blockIdx.x;
        sg.x = rec->band, sg.y = rec->z0, sg.z = rec->z1, sg.w = rec->rows;
#pragma unroll
        for (int k = 0; k < 5; ++k) rec_plane[k] = rec->plane[k];
    };
    request_record();
    asm volatile("" ::"s"(a.pq_partials), "s"(a.pq_nparts), "s"(A.canon_sym_ready), "s"(ntab) : "memory");  // (as in the update walk)
    request_tables();  // (before the sums, as in the update walk)
    if (!FIRST) {
        double s[2] = {0.0, 0.0};
        fold_lane_sums(a.pq_partials, a.pq_nparts, s);
        fold_rho = s[0];
        fold_rr = s[1];
    }
    if (!FIRST && a.it >= stop_iter) return;
    // Prologue, step 2, behind the window requests: tables to LDS, the two cross-wave folds behind one pair of LDS-only
    // barriers, beta.  (The captures are named -- what the step reads, then what it writes -- and keep this order: the
    // compiler's output follows it, down to the order of two assembler comments; profiles/r25_walk_forms.txt.)
    auto tables_and_beta = [&rho_it, &store_tables, &fold_rho, &fold_rr, &cg_rho_new, &cg_rr, &cg_beta, &init_fold]() {
        store_tables();
        if (!FIRST) {
            double v[2] = {fold_rho, fold_rr};
            block_sum_lds(v, red);
            cg_rho_new = v[0];
            cg_rr = v[1];
            cg_beta = cg_rho_new / rho_it;
        }
        init_fold();
        lds_barrier();
    };
    zero_unused_partials<2>(a);
    const int64_t PL = A.sweep_pl;
    const int band = sg.x, z0 = sg.y, z1 = sg.z;
    constexpr bool GEN = RUNS == 0;          // planes that are not whole chunks: byte ids, partial last band (see above)
    const int blen = GEN ? sg.w : T;
    const int64_t gmax = A.ncols - 2;
    const pvd2 du = {a.diag_uniform, a.diag_uniform};
    double acc0 = 0.0;
    typedef const unsigned __attribute__((address_space(4))) *const_words;
    typedef const int __attribute__((address_space(4))) *const_ints;
    if (z0 < z1) {
        const const_ints chain = (const_ints)(uintptr_t)A.chain_plane;
        const const_ints chain_far = (const_ints)(uintptr_t)A.chain_far;
        auto band_row = [&](int z) -> int {  // rows fit 32 bits (the launch is for ncols < 2^28)
            const int k = chain[z];
            return (k < 0 ? 0 : k) * (int)PL + band * T;
        };
        auto clampg = [&](int g) -> int { return clamp_piece(g, gmax); };
        // p' at one 16-byte piece: the expression of dir2 / cg_direction_kernel
        const pvd2 p_scale = {a.p_scale, a.p_scale};  // 1.0 except where a.x is r0 and p0 = p_scale x r0 (virtual p0)
        auto newp = [&](pvd2 rv, pvd2 pv) -> pvd2 {
            const pvd2 zv = a.diag_mode ? du * rv : rv;
            if (FIRST) return zv;
            const pvd2 ps = p_scale * pv;
            pvd2 o;
            o.x = __builtin_fma(cg_beta, ps.x, zv.x);
            o.y = __builtin_fma(cg_beta, ps.y, zv.y);
            return o;
        };
        struct Own {
            pvd2 r[NH], p[NH];
        };
        struct Halo {
            pvd2 r[NHL], p[NHL];
        };
        // (GEN: pieces beyond the band's rows inside the plane repeat its last piece)
        auto piece_of = [&](int k) -> int { return GEN ? min(tid + k * kBlock, blen / 2 - 1) : tid + k * kBlock; };
        auto load_own = [&](int base, Own &o) {
#pragma unroll
            for (int k = 0; k < NH; ++k) {
                const int g = clampg(base + 2 * piece_of(k));
                o.r[k] = *reinterpret_cast<const pvd2 *>(a.cg_r + g);  // (plain: the neighbouring band's halo)
                if (FIRST)
                    o.p[k] = o.r[k];
                else
                    __builtin_memcpy(&o.p[k], a.x + g, 16);
            }
        };
        // p' of the band at a position: to the ring, and to the output vector where the position belongs to
        // the segment
        auto store_own = [&](int z, int base, const Own &o, bool out) {
            double *slot_p = own_ring + (size_t)(z & 3) * T;
#pragma unroll
            for (int k = 0; k < NH; ++k) {
                const pvd2 v = newp(o.r[k], o.p[k]);
                *reinterpret_cast<pvd2 *>(slot_p + 2 * (tid + k * kBlock)) = v;
                // (a.y == nullptr: a direction nobody reads from memory -- windows and sums only)
                if (out && a.y) __builtin_nontemporal_store(v, reinterpret_cast<pvd2 *>(a.y + base + 2 * piece_of(k)));
            }
        };
        auto load_halo = [&](int base, Halo &hh) {
            const int up = base + T;
#pragma unroll
            for (int k = 0; k < NHL; ++k) {
                const int pc = min(tid + k * kBlock, NX / 2 - 1);
                const int g = clampg(up + 2 * pc);
                __builtin_memcpy(&hh.r[k], a.cg_r + g, 16);
                if (FIRST)
                    hh.p[k] = hh.r[k];
                else
                    __builtin_memcpy(&hh.p[k], a.x + g, 16);
            }
        };
        // (the slot of a position is passed in: position modulo 3, kept incrementally)
        auto store_halo = [&](int hslot, const Halo &hh) {
            double *slot_p = halo_ring + (size_t)hslot * NX;
#pragma unroll
            for (int k = 0; k < NHL; ++k) {
                const int pc = min(tid + k * kBlock, NX / 2 - 1);
                *reinterpret_cast<pvd2 *>(slot_p + 2 * pc) = newp(hh.r[k], hh.p[k]);
            }
        };
        struct Rle {
            unsigned w[GEN ? 1 : RUNS / 2];
        };
        auto fetch_rle = [&](int base, int h) -> Rle {
            Rle f;
            if (GEN) {
                f.w[0] = A.pair_id[(base + min(h * kPairRows + 2 * tid, blen - 2)) >> 1];
            } else {
                const const_words q = (const_words)(uintptr_t)(A.pair_rle + ((base + h * kPairRows) / kPairRows) * ((RUNS ? RUNS : 8) / 8));
#pragma unroll
                for (int k = 0; k < (GEN ? 1 : RUNS / 2); ++k) f.w[k] = q[k];
            }
            return f;
        };
        Own own_a, own_b;
        Halo hreg, hreg_b;
        Rle rle_a[NH], rle_b[NH];
        int brow[5];
#pragma unroll
        for (int k = 0; k < 5; ++k)
            brow[k] = (rec_plane[k] < 0 ? 0 : rec_plane[k]) * (int)PL + band * T;  // band_row(z0 - 1 + k), from the record
        SCHWZ_STAMP_AFTER(brow[0] + brow[1] + brow[2] + brow[3] + brow[4]);
        SCHWZ_STAMP(kForm, kStampSegment);
        SCHWZ_STAMP_POSITIONS(z1 - z0);
        {
            // the previous position is read by rows whose far-after slot points backwards along the chain
            Own before, first;
            Halo h0;
            load_own(brow[0], before);
            load_own(brow[1], first);
            load_halo(brow[1], h0);
            load_own(brow[2], own_b);
            load_own(brow[3], own_a);
            // halo of the first position goes to its slot now; the next two stay in flight like the own windows
            load_halo(brow[2], hreg);    // position z0 + 1
            load_halo(brow[3], hreg_b);  // position z0 + 2
            SCHWZ_STAMP_LANDED();
            SCHWZ_STAMP(kForm, kStampWindows);
            tables_and_beta();
            SCHWZ_STAMP(kForm, kStampTables);
            store_halo(0, h0);
            store_own(z0 - 1, brow[0], before, false);
            store_own(z0, brow[1], first, true);
        }
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            rle_a[h] = fetch_rle(brow[1], h);
            rle_b[h] = fetch_rle(z0 + 1 < z1 ? brow[2] : brow[1], h);
        }
        int hs = 0;  // halo slot of the position being computed
        // one position: `own_next` holds r, p of position z + 1 on entry and of position z + 3 on exit, `hal_next`
        // the halo of position z + 1 on entry and of position z + 3 on exit
        auto step = [&](int z, Own &own_next, Rle (&rl)[NH], Halo &hal_next) {
            store_own(z + 1, brow[2], own_next, z + 1 < z1);
            const int hs_next = hs == 2 ? 0 : hs + 1;
            store_halo(hs_next, hal_next);
            lds_barrier();
            load_halo(brow[4], hal_next);
            load_own(brow[4], own_next);
            const int far = chain_far[z];
            const double *cur = own_ring + (size_t)(z & 3) * T;
            const double *prv = own_ring + (size_t)((z + 3) & 3) * T;
            const double *nxt = own_ring + (size_t)((z + 1) & 3) * T;
            const double *hup = halo_ring + (size_t)hs * NX;
            const double *fa0 = far_window(far >> 4, prv, nxt, cur), *fa1 = far_window(far >> 6, prv, nxt, cur);
            const int rbase = z + 2 < z1 ? brow[3] : brow[1];
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const Rle f = rl[h];
                const int i0u = h * kPairRows + 2 * tid;
                const bool valid = !GEN || i0u < blen;
                const int i0 = GEN ? min(i0u, blen - 2) : i0u;
                int pid = GEN ? (int)f.w[0] : (int)((f.w[0] >> 8) & 0xffu);
#pragma unroll
                for (int k = 1; k < RUNS; ++k) {
                    const unsigned e = (f.w[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
                    if ((unsigned)tid >= (e & 0xffu)) pid = (int)(e >> 8);
                }
                pvd2 t[4];
                t[0] = *reinterpret_cast<const pvd2 *>(cur + i0);
                t[1].x = t[0].y;
                t[1].y = i0 + 2 < T ? cur[i0 + 2] : hup[0];
                t[2] = *reinterpret_cast<const pvd2 *>(i0 + NX < T ? cur + (i0 + NX) : hup + (i0 + NX - T));
                t[3] = *reinterpret_cast<const pvd2 *>(fa0 + i0);
                double s0 = 0.0, s1 = 0.0;
                auto add = [&](int k, pvd2 tv) {
                    const PairVal v = cpv[pid * 5 + k];
                    const double p0 = v.a * tv.x, p1 = v.b * tv.y;
                    s0 += p0;
                    s1 += p1;
                };
#pragma unroll
                for (int k = 0; k < 4; ++k) add(k, t[k]);
                if (far & 0xc0) add(4, *reinterpret_cast<const pvd2 *>(fa1 + i0));
                if (GEN) {
                    const double u0 = t[0].x * s0, u1 = t[0].y * s1;
                    acc0 += valid ? u0 : 0.0;
                    acc0 += valid ? u1 : 0.0;
                } else {
                    acc0 += t[0].x * s0;
                    acc0 += t[0].y * s1;
                }
                rl[h] = fetch_rle(rbase, h);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) brow[k] = brow[k + 1];
            brow[4] = band_row(z + 4);
            hs = hs_next;
            if (z == z0) SCHWZ_STAMP(kForm, kStampFirstStep);
        };
        int z = z0;
        for (; z + 1 < z1; z += 2) {
            step(z, own_b, rle_a, hreg);
            step(z + 1, own_a, rle_b, hreg_b);
        }
        if (z < z1) step(z, own_b, rle_a, hreg);
        SCHWZ_STAMP(kForm, kStampLastStep);
    } else if (!FIRST && blockIdx.x == 0) {
        tables_and_beta();  // (an empty first slot still advances the CG state below)
    } else {
        init_fold();  // (... or initialises it)
    }
    const double s0 = block_sum(acc0, red);
    if (tid == 0) {
        a.partials[blockIdx.x] = s0;
        a.partials[a.part_stride + blockIdx.x] = 0.0;
    }
    SCHWZ_STAMP(kForm, kStampDone);
    if (!FIRST && blockIdx.x == 0 && tid == 0) {
        // what cg_direction_kernel's workgroup 0 does
        cg_advance_state(const_cast<CgState *>(a.cg_state), a.it, cg_rho_new, cg_rr, a.cg_rtol);
    }
}

// ---- who may take the z-sweep walk: one definition per launch, asked by launch_spmv_pair and by the CG plan ----

// (dynamic LDS of the walks: sweep_update_lds / sweep_dirdot_lds of coding_plan.hpp, which the plan of the segment
// tables uses too, with this translation unit's kDirdotHaloLines)

// whether a kSpmvCgUpdate launch that leaves x alone (cg_x == nullptr) can take the walk: single-table coding,
// 32-bit byte offsets of x, the Jacobi diagonal absent, a scalar or a full vector, segments and companion
// workgroups within the partial-sum slots, an instantiation for the pieces per lane (own: T / 512, halo:
// NX / 256) and its LDS within the limit
bool pair_sweep_update_ok(const CsrView &A, int grid, int diag_mode)
{
    const int nh = A.sweep_T / kPairRows, nhl = (A.sweep_nx + kBlock - 1) / kBlock;
    return A.pair_single && A.sweep_nslots > 0 && A.ncols < (int64_t(1) << 28) && diag_mode != 2 &&
           A.sweep_nslots + A.sweep_gen_blocks <= grid && (nh == 1 || nh == 2) && nhl <= 4 && A.canon_npat <= kPairPats &&
           sweep_update_lds(A.sweep_T, A.sweep_nx, A.canon_npat) <= kSweepLdsLimit;
}

// ... and the fused direction + p.(A p) launch (kSpmvDirDotSym): a matrix whose update launch walks, symmetric
// tables, the diagonal absent or a scalar, the direction table within the slots, its own instantiations and LDS
bool pair_sweep_dirdot_ok(const CsrView &A, int grid, int diag_mode)
{
    const int nh = A.sweep_T_dir / kPairRows, nhl = (A.sweep_nx / 2 + kBlock - 1) / kBlock;
    return pair_sweep_update_ok(A, grid, diag_mode) && A.canon_sym_ready && diag_mode != 1 &&
           A.sweep_nslots_dir + A.sweep_gen_blocks <= grid && (nh == 1 || nh == 2 || nh == 4) && nhl <= 2 &&
           sweep_dirdot_lds(A.sweep_T_dir, A.sweep_nx, A.canon_npat, kDirdotHaloLines) <= kSweepLdsLimit;
}

// whether a solve on this matrix can START in the z-sweep walk: the INIT form of the update walk and the
// FIRST form of the fused direction walk exist for the shapes both walks take, and only where the walk covers
// every row (no companion launch: cubes and z-slab subdomains); the caller checks the diagonal
bool pair_sweep_start_ok(const CsrView &A, int grid)
{
    return A.sweep_gen_blocks == 0 && pair_sweep_dirdot_ok(A, grid, 0);
}

// ... and with the fused dual residual: the flagged planes' chunk list exists and its launch fits the
// partial-sum slots behind the walk's
bool pair_sweep_dual_ok(const CsrView &A, int grid)
{
    return pair_sweep_start_ok(A, grid) && A.chain_dual && A.dual_chunks && A.dual_blocks > 0 &&
           A.sweep_nslots + A.dual_blocks <= grid;
}

// One instantiation of a z-sweep walk kernel, one workgroup per segment slot: raises its dynamic-LDS limit once,
// launches it.  false: the device does not grant 96 KiB of dynamic LDS to the kernel (nothing was launched).
#ifdef SCHWZ_WITH_PROBES
// the timeline buffer of the measurement build: kMaxGrid records of kWalkStampWords words for each of the next
// `launches` walk launches, in launch order (tools/walk_timeline.py owns and zeroes the memory)
static unsigned long long *g_walk_probe = nullptr;
static int g_walk_probe_cap = 0, g_walk_probe_used = 0;
extern "C" void schwz_walk_probe_set(unsigned long long *dev_buf, int launches)
{
    g_walk_probe = dev_buf;
    g_walk_probe_cap = dev_buf ? launches : 0;
    g_walk_probe_used = 0;
}
extern "C" int schwz_walk_probe_used() { return g_walk_probe_used; }
extern "C" int schwz_walk_probe_record_words() { return kWalkStampWords; }
extern "C" int schwz_walk_probe_launch_records() { return kMaxGrid; }
#endif

template <void (*KERNEL)(CsrView, SpmvArgs)>
static bool launch_walk_kernel(int nslots, const CsrView &A, const SpmvArgs &b, size_t lds, hipStream_t s)
{
    static const hipError_t e = hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    kSweepLdsLimit);
    if (e != hipSuccess || lds > kSweepLdsLimit) return false;
#ifdef SCHWZ_WITH_PROBES
    if (g_walk_probe_used < g_walk_probe_cap && nslots <= kMaxGrid) {
        SpmvArgs c = b;
        c.walk_probe = g_walk_probe + (size_t)g_walk_probe_used++ * kMaxGrid * kWalkStampWords;
        hipLaunchKernelGGL(KERNEL, dim3(nslots), dim3(kBlock), lds, s, A, c);
        return true;
    }
#endif
    hipLaunchKernelGGL(KERNEL, dim3(nslots), dim3(kBlock), lds, s, A, b);
    return true;
}

// The update / start walk: the instantiation by the run-length record of the matrix (8 / 16 runs per chunk)
template <int L_, int H_, bool DV, bool INIT, bool DUAL>
static bool launch_sweep_variant(const CsrView &A, const SpmvArgs &b, size_t lds, hipStream_t s)
{
    if (A.sweep_gen_mode) {
        // planes that are not whole chunks (byte ids, partial last band); no dual form there
        if (DUAL) return false;
        return launch_walk_kernel<spmv_pair_sweep_kernel<L_, H_, DV, INIT, false, 0>>(A.sweep_nslots, A, b, lds, s);
    }
    return A.pair_rle_runs == 16
               ? launch_walk_kernel<spmv_pair_sweep_kernel<L_, H_, DV, INIT, DUAL, 16>>(A.sweep_nslots, A, b, lds, s)
               : launch_walk_kernel<spmv_pair_sweep_kernel<L_, H_, DV, INIT, DUAL, 8>>(A.sweep_nslots, A, b, lds, s);
}

// ... and by the halo / own pieces per lane (pair_sweep_update_ok has checked that the instantiation exists)
template <bool DV, bool INIT, bool DUAL>
static bool launch_update_walk(const CsrView &A, const SpmvArgs &b, hipStream_t s)
{
    const int nhl = (A.sweep_nx + kBlock - 1) / kBlock, nh = A.sweep_T / kPairRows;
    const size_t lds = sweep_update_lds(A.sweep_T, A.sweep_nx, A.canon_npat);
    if (nh == 1)
        return nhl == 1   ? launch_sweep_variant<1, 1, DV, INIT, DUAL>(A, b, lds, s)
               : nhl == 2 ? launch_sweep_variant<2, 1, DV, INIT, DUAL>(A, b, lds, s)
                          : launch_sweep_variant<4, 1, DV, INIT, DUAL>(A, b, lds, s);
    return nhl == 1   ? launch_sweep_variant<1, 2, DV, INIT, DUAL>(A, b, lds, s)
           : nhl == 2 ? launch_sweep_variant<2, 2, DV, INIT, DUAL>(A, b, lds, s)
                      : launch_sweep_variant<4, 2, DV, INIT, DUAL>(A, b, lds, s);
}

// The same two steps for the fused direction walk (FIRST: the first direction of a solve that started in
// the walk) over the direction table of the view it is given.
template <int L_, int H_, bool FIRST>
static bool launch_dirdot_variant(const CsrView &A, const SpmvArgs &b, size_t lds, hipStream_t s)
{
    const int nslots = A.sweep_nslots_dir;
    if (A.sweep_gen_mode) return launch_walk_kernel<spmv_pair_dirdot_sweep_kernel<L_, H_, FIRST, 0>>(nslots, A, b, lds, s);
    return A.pair_rle_runs == 16 ? launch_walk_kernel<spmv_pair_dirdot_sweep_kernel<L_, H_, FIRST, 16>>(nslots, A, b, lds, s)
                                 : launch_walk_kernel<spmv_pair_dirdot_sweep_kernel<L_, H_, FIRST, 8>>(nslots, A, b, lds, s);
}

template <bool FIRST>
static bool launch_dirdot_walk(const CsrView &A, const SpmvArgs &b, hipStream_t s)
{
    const int nhl = (A.sweep_nx / 2 + kBlock - 1) / kBlock, nh = A.sweep_T_dir / kPairRows;
    const size_t lds = sweep_dirdot_lds(A.sweep_T_dir, A.sweep_nx, A.canon_npat, kDirdotHaloLines);
    if (nh == 1)
        return nhl == 1 ? launch_dirdot_variant<1, 1, FIRST>(A, b, lds, s) : launch_dirdot_variant<2, 1, FIRST>(A, b, lds, s);
    if (nh == 2)
        return nhl == 1 ? launch_dirdot_variant<1, 2, FIRST>(A, b, lds, s) : launch_dirdot_variant<2, 2, FIRST>(A, b, lds, s);
    return nhl == 1 ? launch_dirdot_variant<1, 4, FIRST>(A, b, lds, s) : launch_dirdot_variant<2, 4, FIRST>(A, b, lds, s);
}

int launch_spmv_pair(const CsrView &A, int mode, const SpmvArgs &a, int grid, hipStream_t s)
{
    const bool wide = A.ncols >= (int64_t(1) << 28);  // byte offsets of x beyond 32 bits
    const char *const no_lds = "launch_spmv_pair: the z-sweep kernels cannot have 96 KiB of dynamic LDS on this device";
    if ((mode == kSpmvResidInit || mode == kSpmvResidDual) && a.sweep_init) {
        // CG start in the z-sweep walk (pcg_begin asks for it only where pair_sweep_start_ok holds and the
        // Jacobi diagonal is a scalar or absent): r = b - A x to a.y, partial r.z and r.r; p is not written
        if (!pair_sweep_start_ok(A, grid) || a.diag_mode == 1 || a.diag_mode == 2 || a.dinv) {
            set_error("launch_spmv_pair: the z-sweep start launch does not apply to this matrix");
            return SCHWZ_ERR_INVALID;
        }
        SpmvArgs b = a;
        b.part_stride = grid;
        b.part_offset = 0;
        // fused check residual on a second vector (a subdomain with neighbours): the planes where it needs its
        // own product are left out of the third partial bank here and added by a listed launch below
        const bool with_dual = mode == kSpmvResidDual && a.x2 != nullptr;
        if (with_dual && !pair_sweep_dual_ok(A, grid)) {
            set_error("launch_spmv_pair: the z-sweep dual start launch does not apply to this matrix");
            return SCHWZ_ERR_INVALID;
        }
        if (!(with_dual ? launch_update_walk<false, true, true>(A, b, s) : launch_update_walk<false, true, false>(A, b, s))) {
            set_error(no_lds);
            return SCHWZ_ERR_HIP;
        }
        SCHWZ_HIP_TRY(hipGetLastError());
        if (with_dual) {
            // ||b - A x2||^2 over the flagged planes: chunk by chunk on x2, partial sums into the third bank
            // behind the walk's (the launch also writes zeros into the same slots of the second bank)
            SpmvArgs c;
            c.x = a.x2;
            c.b = a.b;
            c.row_limit = a.row_limit;
            c.sweep = 2;
            c.partials = a.partials + grid;
            c.part_stride = grid;
            c.part_offset = A.sweep_nslots;
            hipLaunchKernelGGL((spmv_pair_kernel<kSpmvResidNorm, false, true>), dim3(A.dual_blocks), dim3(kBlock),
                               kPairTableLds, s, A, c);
            SCHWZ_HIP_TRY(hipGetLastError());
        }
        return SCHWZ_OK;
    }
    if (mode == kSpmvDirDotSym && a.sweep_first) {
        // first direction of such a solve: p' = D^-1 r and the partial sums of p'.(A p'), CgState untouched
        if (!pair_sweep_start_ok(A, grid) || a.diag_mode == 1 || a.diag_mode == 2) {
            set_error("launch_spmv_pair: the z-sweep first-direction launch does not apply to this matrix");
            return SCHWZ_ERR_INVALID;
        }
        // (the kernel reads its records from sweep_rec_dir: this launch gets a view whose direction table IS the
        // first-direction table)
        CsrView Af = A;
        if (A.sweep_rec_first && A.sweep_nslots_first <= grid) {
            Af.sweep_T_dir = A.sweep_T_first;
            Af.sweep_rec_dir = A.sweep_rec_first;
            Af.sweep_nslots_dir = A.sweep_nslots_first;
        }
        SpmvArgs b = a;
        b.part_stride = grid;
        b.part_offset = 0;
        if (!launch_dirdot_walk<true>(Af, b, s)) {
            set_error(no_lds);
            return SCHWZ_ERR_HIP;
        }
        SCHWZ_HIP_TRY(hipGetLastError());
        return SCHWZ_OK;
    }
    // a.walk: whoever planned the launch (the plan of a CG solve in cg.hip, from the same predicates) wants the walk.  A plan the matrix
    // cannot serve is an error; the one thing only this function can find out is the device refusing the LDS.
    if ((mode == kSpmvCgUpdate && a.walk && (a.cg_x || !pair_sweep_update_ok(A, grid, a.diag_mode))) ||
        (mode == kSpmvDirDotSym && a.walk && !pair_sweep_dirdot_ok(A, grid, a.diag_mode))) {
        set_error("launch_spmv_pair: a launch planned for the z-sweep walk cannot take it on this matrix");
        return SCHWZ_ERR_INVALID;
    }
    if (mode == kSpmvCgUpdate && a.walk) {
        // z-sweep walk + (where boundary planes or overlap rows exist) the listed walk of the chunks it
        // leaves out; the consumer folds `grid` partial sums per bank, as after a chunk-by-chunk launch
        SpmvArgs b = a;
        b.part_stride = grid;
        b.part_offset = A.sweep_gen_blocks;  // slots of the companion launch follow this one's
        // false: no LDS for the instantiation -- chunk by chunk then
        if (a.diag_mode == 1 ? launch_update_walk<true, false, false>(A, b, s) : launch_update_walk<false, false, false>(A, b, s)) {
            SCHWZ_HIP_TRY(hipGetLastError());
            if (A.sweep_gen_blocks > 0) {
                SpmvArgs c = a;
                c.sweep = 1;
                c.part_stride = grid;
                c.part_offset = A.sweep_nslots;
                hipLaunchKernelGGL((spmv_pair_kernel<kSpmvCgUpdate, false, true>), dim3(A.sweep_gen_blocks), dim3(kBlock),
                                   kPairTableLds, s, A, c);
                SCHWZ_HIP_TRY(hipGetLastError());
            }
            return SCHWZ_OK;
        }
    }
    if (mode == kSpmvDirDotSym && a.walk) {
        // the companion first: the z-sweep kernel's workgroup 0 advances CgState for both
        if (A.sweep_gen_blocks > 0) {
            SpmvArgs c = a;
            c.sweep = 1;
            c.part_stride = grid;
            c.part_offset = A.sweep_nslots_dir;
            hipLaunchKernelGGL((spmv_pair_kernel<kSpmvDirDotSym, false, true>), dim3(A.sweep_gen_blocks), dim3(kBlock),
                               kPairTableLds, s, A, c);
            SCHWZ_HIP_TRY(hipGetLastError());
        }
        SpmvArgs b = a;
        b.part_stride = grid;
        b.part_offset = A.sweep_gen_blocks;
        if (!launch_dirdot_walk<false>(A, b, s)) {
            set_error(no_lds);
            return SCHWZ_ERR_HIP;
        }
        SCHWZ_HIP_TRY(hipGetLastError());
        return SCHWZ_OK;
    }
    if (a.p0_virtual) {
        // (the chunk-by-chunk kernels read a stored p0; pcg_iterate only asks for the virtual one where the walks apply)
        set_error("launch_spmv_pair: a launch on the virtual first direction was not served by the z-sweep walk");
        return SCHWZ_ERR_INVALID;
    }
#define SCHWZ_PAIR_LAUNCH(M)                                                                          \
    if (wide)                                                                                         \
        hipLaunchKernelGGL((spmv_pair_kernel<M, true, false>), dim3(grid), dim3(kBlock), kPairTableLds, s, A, a);  \
    else if (A.pair_single)                                                                           \
        hipLaunchKernelGGL((spmv_pair_kernel<M, false, true>), dim3(grid), dim3(kBlock), kPairTableLds, s, A, a);  \
    else                                                                                              \
        hipLaunchKernelGGL((spmv_pair_kernel<M, false, false>), dim3(grid), dim3(kBlock), kPairTableLds, s, A, a);
    switch (mode) {
    case kSpmvPlain: SCHWZ_PAIR_LAUNCH(kSpmvPlain) break;
    case kSpmvDot: SCHWZ_PAIR_LAUNCH(kSpmvDot) break;
    case kSpmvResidInit: SCHWZ_PAIR_LAUNCH(kSpmvResidInit) break;
    case kSpmvResidDual: SCHWZ_PAIR_LAUNCH(kSpmvResidDual) break;
    case kSpmvDotOnly: SCHWZ_PAIR_LAUNCH(kSpmvDotOnly) break;
    case kSpmvDotSym: SCHWZ_PAIR_LAUNCH(kSpmvDotSym) break;
    case kSpmvDirDotSym: SCHWZ_PAIR_LAUNCH(kSpmvDirDotSym) break;
    case kSpmvDirDotSymVec: SCHWZ_PAIR_LAUNCH(kSpmvDirDotSymVec) break;
    case kSpmvCgUpdate: SCHWZ_PAIR_LAUNCH(kSpmvCgUpdate) break;
    default: SCHWZ_PAIR_LAUNCH(kSpmvResidNorm) break;
    }
#undef SCHWZ_PAIR_LAUNCH
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

// ---- uploads: the plans of coding_plan.hpp become device arrays bound to CsrView; nothing is decided here ----

// the pair fields of A->v from a plan and the arrays uploaded for it (a fresh plan, no arrays: not pair coded)
static void bind_pair(schwz_csr *A, const PairPlan &P)
{
    CsrView &v = A->v;
    const auto &b = A->coding.pair;
    v.pair_id = b.pair_id.as<uint8_t>();
    v.pair_rle = b.rle.as<uint4>();
    v.pair_rle_runs = P.rle_runs;
    v.chunk_ptable = b.chunk_ptable.as<schwz_idx>();
    v.ptbl_desc = b.ptbl_desc.as<schwz_idx>();
    v.ptbl_len = b.ptbl_len.as<uint8_t>();
    v.ptbl_val = b.ptbl_val.as<double>();
    v.ptbl_meta = b.ptbl_meta.as<schwz_idx>();
    v.pair_single = P.single;
    std::copy(P.canon, P.canon + 8, v.pair_canon);
    v.pair_sym_base = P.sym_base;
    v.pair_shift = P.shift;
    A->pair_fraction = P.fraction;
    A->pair_code_bytes = P.code_bytes;
}

// ... the z-sweep walk's; a launch without records of its own reads the table before it
static void bind_walk(schwz_csr *A, const WalkPlan &W)
{
    CsrView &v = A->v;
    const auto &b = A->coding.walk;
    v.sweep_gen_mode = W.gen_mode;
    v.sweep_T = W.T;
    v.sweep_nx = W.nx;
    v.sweep_pl = W.pl;
    v.sweep_nslots = W.nslots();
    v.sweep_ngen = (int)W.gen.size();
    v.sweep_gen_blocks = W.gen_blocks;
    v.sweep_gen = b.gen.as<schwz_idx>();
    v.sweep_T_dir = W.T_dir;
    v.sweep_nslots_dir = W.nslots_dir();
    v.sweep_T_first = W.T_first;
    v.sweep_nslots_first = W.nslots_first();
    v.canon_npat = W.npat;
    v.chain_plane = b.chain_plane.as<int>();
    v.chain_far = b.chain_far.as<int>();
    v.sweep_rec = b.rec.as<WalkRecord>();
    v.sweep_rec_dir = b.rec_dir.p ? b.rec_dir.as<WalkRecord>() : v.sweep_rec;
    v.sweep_rec_first = b.rec_first.p ? b.rec_first.as<WalkRecord>() : v.sweep_rec_dir;
    v.canon_ready = b.canon_ready.as<double>();
    v.canon_sym_ready = b.canon_sym_ready.as<double>();
    A->h_chain_plane = W.chain_plane;
}

// ... and the fused dual residual's
static void bind_dual(schwz_csr *A, const DualPlan &D)
{
    const auto &b = A->coding.dual;
    A->v.chunk_dual = b.chunk_dual.as<uint8_t>();
    A->v.chain_dual = b.chain_dual.as<int>();
    A->v.dual_chunks = b.dual_chunks.as<schwz_idx>();
    A->v.dual_nchunks = (int)D.dual_chunks.size();
    A->v.dual_blocks = D.dual_blocks;
}

static int upload_walk(schwz_csr *A, const WalkPlan &W)
{
    if (!W.built()) return SCHWZ_OK;
    auto &b = A->coding.walk;
    int rc = SCHWZ_OK;
    // what the kernels read: the companion's chunk list, the chains, and at entry the records and the ready tables
    // (the plan's segment tables, values and masks, from which those are derived, stay on the host)
    if ((rc = b.gen.put(W.gen)) || (rc = b.chain_plane.put(W.chain_plane)) || (rc = b.chain_far.put(W.chain_far)))
        return rc;
    if ((!W.rec_dir.empty() && (rc = b.rec_dir.put(W.rec_dir))) || (!W.rec_first.empty() && (rc = b.rec_first.put(W.rec_first))) ||
        (rc = b.rec.put(W.rec)) || (rc = b.canon_ready.put(W.canon_ready)) ||
        (!W.canon_sym_ready.empty() && (rc = b.canon_sym_ready.put(W.canon_sym_ready))))
        return rc;
    return SCHWZ_OK;
}

// Row pairs and, over a single-table coding, the z-sweep walk.  On an error the caller releases the codings.
int build_spmv_pair(schwz_csr *A, const CodingOptions &opt, const HostCsr &M)
{
    PairPlan P;
    if (!plan_pair_tables(opt, M, P)) {
        A->pair_fraction = P.fraction;
        return SCHWZ_OK;
    }
    StageTimer t_rest("  pairs: tables, records, canonical layout, walk tables, uploads");
    plan_pair_records(opt, M, A->pair_deal_shift, P);
    // the segment lengths follow the number of CUs: asked here, the plan takes it as a number -- and only where the
    // plan can get as far as its segments (a canonical layout, run-length records, the walk not switched off)
    int cus = 256, dev = 0;
    hipDeviceProp_t prop;
    if (P.single && P.canon[7] && !P.rle.empty() && opt.sweep != 0 && hipGetDevice(&dev) == hipSuccess &&
        hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        cus = prop.multiProcessorCount;
    const WalkPlan W = plan_walk(opt, P, M.nrows, M.ncols, walk_grid((int64_t)M.tiles.size() - 1), cus, kDirdotHaloLines);
    // SCHWZ_SWEEP_WHY=1: says on stderr why a matrix gets no z-sweep walk
    if (opt.sweep_why && !W.why.empty()) std::fprintf(stderr, "[schwz] no z-sweep walk: %s\n", W.why.c_str());
    auto &b = A->coding.pair;
    int rc = SCHWZ_OK;
    if ((rc = b.pair_id.put(P.pair_id)) || (rc = b.chunk_ptable.put(P.chunk_ptable)) || (rc = b.ptbl_desc.put(P.ptbl_desc)) ||
        (rc = b.ptbl_len.put(P.ptbl_len)) || (rc = b.ptbl_val.put(P.ptbl_val)) || (rc = b.ptbl_meta.put(P.ptbl_meta)) ||
        (!P.rle.empty() && (rc = b.rle.put(P.rle))) || (rc = upload_walk(A, W)))
        return rc;
    bind_pair(A, P);
    bind_walk(A, W);
    return SCHWZ_OK;
}

// chunks whose rows or columns reach `split` need the second product of the fused dual residual: planned
// again on every call, the three arrays replaced
int pair_set_dual_split(schwz_csr *A, const schwz_idx *h_rp, const schwz_idx *h_col, int64_t split)
{
    if (!A->v.pair_id) return SCHWZ_OK;
    const bool whole_chunk_walk = A->v.sweep_nslots > 0 && !A->v.sweep_gen_mode;
    const DualPlan D = plan_dual_split(A->v.nrows, h_rp, h_col, split, A->h_chain_plane, whole_chunk_walk ? A->v.sweep_pl : 0);
    auto &b = A->coding.dual;
    b = {};
    int rc = b.chunk_dual.put(D.chunk_dual);
    if (!rc && !D.dual_chunks.empty() && !(rc = b.chain_dual.put(D.chain_dual))) rc = b.dual_chunks.put(D.dual_chunks);
    if (rc) b = {};
    bind_dual(A, rc ? DualPlan() : D);
    return rc;
}

void free_spmv_pair(schwz_csr *A)
{
    A->coding.pair = {};
    A->coding.walk = {};
    A->coding.dual = {};
    bind_pair(A, PairPlan());
    bind_walk(A, WalkPlan());
    bind_dual(A, DualPlan());
}

}  // namespace schwz
