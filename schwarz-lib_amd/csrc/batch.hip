// Block vectors: K right-hand sides against one matrix (an extension, include/schwz_hip.h "Block vectors").
//
// A block vector of n rows and K columns is stored row-interleaved, element (i, j) at i * K + j, K = 2, 4 or 8: the
// K operands a matrix entry a_ic needs are the 8 K contiguous bytes at X + c * K, and a vector kernel that walks the
// n * K elements in order has its column fixed per lane (256 = 0 mod K): lane t works on column t % K throughout.
//
// batch_spmm_kernel: plain CSR, whatever coding the upload chose for the single-vector path, over the tiles of
// CsrView (tile_row, tile_nz).  A workgroup stages the values and columns of a tile in LDS with 16-byte loads --
// once per tile, independent of K -- and then K adjacent lanes are one row: they read the same staged entry (an LDS
// broadcast) and gather the K operands of its column in one contiguous access; 256 / K rows per pass.  Row sums run
// in CSR order with contraction off, like every other SpMV of the library.  A tile that does not fit the window (a
// row of more than ~2048 entries is a tile of its own) is summed straight from HBM by the same lanes: built for
// correctness only.  The epilogues are those the block CG and the RAS step need; their sums are per column, one
// partial sum per workgroup (vector launches: per team of 32 rows) and column, folded by the NEXT launch in a fixed
// order (the fold_partials idiom: no atomics, no fences, no ticket counters) that does not depend on K (team_sum).
//
// schwz_bcg: K independent CG recurrences that share the matrix pass.  alpha_j, beta_j and the freeze mask live in
// BcgState on the device; three launches per iteration (Q = A P; update of x, r; direction).  A column is frozen --
// its x, r and p stop changing, bit for bit -- once ||r_j|| <= rtol ||r_0,j||, or where r_0 = 0, p.q = 0 or r.z = 0
// would be divided by, or from the first launch on by the caller's mask.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <limits>
#include <vector>

#include "schwz_internal.hpp"
#include "device_utils.hpp"
#include "stream_pipeline.hpp"

namespace schwz {

constexpr int kBatchMaxK = 8;
// Workgroups per launch: every workgroup of the next launch folds K (or 2 K) partial sums per workgroup of this one,
// so the grids stay at four workgroups per CU and stride beyond.
constexpr int kBatchGrid = 1024;
// the staged window of a tile: at most kTileNnz entries behind a 16-byte aligned start, in whole quads
constexpr int kBatchLds = kTileNnz + 8;

enum BatchMode {
    kBatchPlain = 0,      // Y = alpha A X + beta Y
    kBatchDot = 1,        // Q = A P ; per column partial sums of p.q
    kBatchResidInit = 2,  // R = B - A X ; P = M^-1 R ; per column partial sums of r.z and r.r
    kBatchResid = 3,      // R = B - A X ; per column partial sums of r.r
    kBatchResidNorm = 4   // per column partial sums of (b - A x)^2, nothing stored
};

// The scalars of the K recurrences.  rho and frozen have two slots: the direction launch of iteration `it` reads slot
// it & 1 in every workgroup while its workgroup 0 writes the other one.
struct BcgState {
    double rho[2][kBatchMaxK];
    double rr[kBatchMaxK];  // ||r_j||^2 of the recurrence, as of the column's last update
    double r0[kBatchMaxK];  // ||r_0,j||
    int iters[kBatchMaxK];  // updates applied to column j
    unsigned frozen[2];     // bit j: column j takes no further update (start and direction launches write it)
    unsigned frozen_upd;    // ... and the columns whose p.q = 0 the update launch of the running iteration found
    int stop_iter;          // INT_MAX until every column is frozen (what the host polls)
};

struct BatchArgs {
    double alpha = 1.0, beta = 0.0;
    const double *x = nullptr;  // the gathered block vector (X / P)
    double *y = nullptr;        // Y / Q / R
    const double *b = nullptr;  // B of the residual forms
    double *p = nullptr;        // kBatchResidInit: first direction out
    const double *dinv = nullptr;
    double *part = nullptr;  // [gridDim.x][K] per bank; kBatchDot fills one bank, the residual forms two
    const BcgState *st = nullptr;
    int it = 0;
    int64_t row_limit = INT64_MAX;  // kBatchResidNorm: rows >= row_limit add nothing to the sums
};

// The order of every sum over rows is the same for K = 2, 4 and 8, so that a column's numbers do not depend on the
// width of the block it travels in (a run of 3 columns, padded to 4, gives the bits of the same columns in a block of
// 8).  The unit is a TEAM: kTeamRows = 32 row slots times K columns, lane t of a workgroup being column t % K of row
// slot (t / K) % 32 of team t / (32 K); a workgroup holds 8 / K teams (one at K = 8).  A lane adds what belongs to
// its row slot in ascending row order; team_sum then adds the 32 row slots of a team as a tree over the slot's bits
// 2, 1, 0 inside the wave and ((g0 + g1) + (g2 + g3)) over its four groups of eight slots.  Nothing in that depends on K.
constexpr int kTeamRows = 32;

// `red` holds 32 doubles; the result of team `team` (0 .. 8 / K - 1), valid in every lane that asks for it
template <int K>
__device__ __forceinline__ double team_sum(double v, double *red, int team)
{
#pragma unroll
    for (int off = 4 * K; off >= K; off >>= 1) v += __shfl_xor(v, off, 64);
    const int c = threadIdx.x / K, j = threadIdx.x % K;
    __syncthreads();  // protect `red` from a previous use
    if ((c & 7) == 0) red[(c >> 3) * K + j] = v;
    __syncthreads();
    const double *g = red + 4 * team * K;
    return (g[j] + g[K + j]) + (g[2 * K + j] + g[3 * K + j]);
}

// The partial sums [nparts][K] a launch left, folded per column by team 0 -- row slot c adds the partial sums c,
// c + 32, ... in that order --; every workgroup folds them itself, and every lane gets its column's sum.
template <int K>
__device__ __forceinline__ double col_fold(const double *part, int nparts, double *red)
{
    const int c = threadIdx.x / K, j = threadIdx.x % K;
    double s = 0.0;
    if (c < kTeamRows) {
#pragma unroll 4
        for (int i = c; i < nparts; i += kTeamRows) s += part[(size_t)i * K + j];
    }
    return team_sum<K>(s, red, 0);
}

// slot `at` of `nparts` of bank 0 and, with TWO, of bank 1 (nparts * K doubles on), by the K lanes that hold the sums
template <int K, bool TWO>
__device__ __forceinline__ void col_store_partials(double s0, double s1, double *part, int at, int nparts)
{
    part[(size_t)at * K + threadIdx.x % K] = s0;
    if (TWO) part[((size_t)nparts + at) * K + threadIdx.x % K] = s1;
}

template <int K, int MODE>
__global__ __launch_bounds__(kBlock) void batch_spmm_kernel(CsrView A, BatchArgs a)
{
#pragma clang fp contract(off)
    // the staged entries of a tile; once its row sums are done, the per-row terms of the fused sums (kTileRows x K)
    __shared__ __attribute__((aligned(16))) double vals[kBatchLds];
    __shared__ __attribute__((aligned(16))) int cols[kBatchLds];
    __shared__ int rstart[kTileRows + 1];  // first entry of every row of the tile, window-relative
    __shared__ double terms1[MODE == kBatchResidInit ? kTileRows * K : 1];  // ... of the second sum (r.r beside r.z)
    __shared__ double red[32];
    static_assert(kTileRows * K <= kBatchLds, "the per-row terms of a tile fit the staging array");
    constexpr unsigned kFull = (1u << K) - 1u;
    constexpr int kRows = kBlock / K;  // rows per pass; K passes cover the kTileRows rows of a chunk
    constexpr bool kTwo = MODE == kBatchResidInit;
    if (MODE == kBatchDot && (a.st->frozen[a.it & 1] & kFull) == kFull) return;  // (written by an earlier launch)
    const int tid = threadIdx.x, j = tid % K, slot = tid / K;
    // the fused sums: kBatchDot p.q; kBatchResidInit r.z and r.r; kBatchResid / kBatchResidNorm r.r
    double acc0 = 0.0, acc1 = 0.0;
    for (int t = blockIdx.x; t < A.ntiles; t += gridDim.x) {
        const int r0 = A.tile_row[t], nr = A.tile_row[t + 1] - r0;
        const int s = A.tile_nz[t], e = A.tile_nz[t + 1];
        const int s2 = s & ~3, nq = (e - s2 + 3) >> 2;
        const bool staged = 4 * nq <= kBatchLds && nr <= kTileRows;  // the same for every lane
        __syncthreads();  // every lane is done with the previous tile's entries and terms
        if (staged) {
            // (the last quad may reach three entries past the matrix: the upload pads val and col by four)
            for (int q = tid; q < nq; q += kBlock) {
                ValueQuad<double> v;
                v.load(A.val + s2 + 4 * q);
                v.store(&vals[4 * q]);
                *reinterpret_cast<vi4 *>(&cols[4 * q]) = *reinterpret_cast<const vi4 *>(A.col + s2 + 4 * q);
            }
            for (int i = tid; i <= nr; i += kBlock) rstart[i] = A.rp[r0 + i] - s2;
            __syncthreads();
        }
        // chunks of kTileRows rows: one, unless a tile ever holds more rows (then it is not staged)
        for (int base = 0; base < nr; base += kTileRows) {
            double t0[K], t1[K];
#pragma unroll
            for (int p = 0; p < K; ++p) {
                const int rl = base + slot + p * kRows;
                t0[p] = t1[p] = 0.0;
                if (rl < nr) {
                    const int row = r0 + rl;
                    double sum = 0.0;
                    if (staged) {
                        const int b1 = rstart[rl + 1];
                        int i = rstart[rl];
                        for (; i + 4 <= b1; i += 4) {
                            double vv[4], xx[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                vv[u] = vals[i + u];
                                xx[u] = a.x[(int64_t)cols[i + u] * K + j];
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const double pv = vv[u] * xx[u];
                                sum += pv;
                            }
                        }
                        for (; i < b1; ++i) {
                            const double pv = vals[i] * a.x[(int64_t)cols[i] * K + j];
                            sum += pv;
                        }
                    } else {
                        const int b1 = A.rp[row + 1];
                        for (int i = A.rp[row]; i < b1; ++i) {
                            const double pv = A.val[i] * a.x[(int64_t)A.col[i] * K + j];
                            sum += pv;
                        }
                    }
                    const int64_t o = (int64_t)row * K + j;
                    if (MODE == kBatchPlain) {
                        const double as = a.alpha * sum;
                        if (a.beta != 0.0) {
                            const double by = a.beta * a.y[o];
                            a.y[o] = as + by;
                        } else {
                            a.y[o] = as;
                        }
                    } else if (MODE == kBatchDot) {
                        a.y[o] = sum;
                        t0[p] = a.x[o] * sum;
                    } else {
                        const double r = a.b[o] - sum;
                        const double rr = r * r;
                        if (MODE == kBatchResidInit) {
                            const double z = a.dinv ? a.dinv[row] * r : r;
                            a.y[o] = r;
                            a.p[o] = z;
                            t0[p] = r * z;
                            t1[p] = rr;
                        } else {
                            if (MODE == kBatchResid) a.y[o] = r;
                            t0[p] = (MODE != kBatchResidNorm || row < a.row_limit) ? rr : 0.0;
                        }
                    }
                }
            }
            if (MODE != kBatchPlain) {
                // the terms of the chunk's rows go through LDS, so that row slot c of team 0 can add those of the rows
                // c, c + 32, ... in that order, whatever K is
                __syncthreads();  // every lane is done with the staged entries
#pragma unroll
                for (int p = 0; p < K; ++p) {
                    vals[(slot + p * kRows) * K + j] = t0[p];
                    if (kTwo) terms1[(slot + p * kRows) * K + j] = t1[p];
                }
                __syncthreads();
                if (slot < kTeamRows) {
                    const int nrc = min(nr - base, kTileRows);
                    for (int rl = slot; rl < nrc; rl += kTeamRows) {
                        acc0 += vals[rl * K + j];
                        if (kTwo) acc1 += terms1[rl * K + j];
                    }
                }
                if (base + kTileRows < nr) __syncthreads();  // (the next chunk's terms overwrite these)
            }
        }
    }
    if (MODE != kBatchPlain) {
        const double s0 = team_sum<K>(acc0, red, 0);
        const double s1 = kTwo ? team_sum<K>(acc1, red, 0) : 0.0;
        if (tid < K) col_store_partials<K, kTwo>(s0, s1, a.part, blockIdx.x, gridDim.x);
    }
}

// per column: out[j] = the fold of the partial sums (one workgroup)
template <int K>
__global__ __launch_bounds__(kBlock) void batch_fold_kernel(const double *part, int nparts, double *out)
{
    __shared__ double red[32];
    const double v = col_fold<K>(part, nparts, red);
    if (threadIdx.x < K) out[threadIdx.x] = v;
}

// Start of a solve (one workgroup): the partial sums of the kBatchResidInit launch folded into the state.  A column
// is frozen from the start by the caller's mask, by the loop-top test of iteration 0 and where rho = r.z = 0.
template <int K>
__global__ __launch_bounds__(kBlock) void bcg_start_kernel(BcgState *st, const double *part, int nparts, double rtol,
                                                           unsigned frozen)
{
    __shared__ double red[32];
    constexpr unsigned kFull = (1u << K) - 1u;
    const double rho = col_fold<K>(part, nparts, red);
    const double rr = col_fold<K>(part + (size_t)nparts * K, nparts, red);
    if (threadIdx.x < 64) {
        const int j = threadIdx.x;  // (lanes >= K repeat column j % K and store nothing)
        const double nrm = sqrt(rr);
        const bool fz = ((frozen >> (j % K)) & 1u) || nrm <= rtol * nrm || rho == 0.0;
        const unsigned mask = (unsigned)__ballot(fz) & kFull;
        if (j < K) {
            st->rho[0][j] = rho;
            st->rho[1][j] = 0.0;
            st->rr[j] = rr;
            st->r0[j] = nrm;
            st->iters[j] = 0;
        }
        if (j == 0) {
            st->frozen[0] = mask;
            st->frozen[1] = mask;
            st->frozen_upd = mask;
            st->stop_iter = mask == kFull ? 0 : INT_MAX;
        }
    }
}

// The vector launches walk the rows in teams: team w of `nteams` takes the groups of 32 rows w, w + nteams, ..., and a
// workgroup holds the 8 / K teams blockIdx.x * (8 / K) + 0 .. -- adjacent groups, so its accesses stay contiguous.
// nteams depends on the number of rows alone (batch_teams), and so does every sum.

// x_j += alpha_j p_j, r_j -= alpha_j q_j for the columns that are not frozen, alpha_j = rho_j / (p_j.q_j) from the
// folded partial sums of the Q = A P launch; per column and team partial sums of r.z and r.r of the new residual.
template <int K>
__global__ __launch_bounds__(kBlock) void bcg_update_kernel(int64_t nrows, int nteams, BcgState *st, int it,
                                                            const double *pq_part, int pq_nparts, double *__restrict__ x,
                                                            double *__restrict__ r, const double *__restrict__ p,
                                                            const double *__restrict__ q, const double *__restrict__ dinv,
                                                            double *part)
{
#pragma clang fp contract(off)
    __shared__ double red[32];
    constexpr unsigned kFull = (1u << K) - 1u;
    const unsigned fz = st->frozen[it & 1];
    if ((fz & kFull) == kFull) return;
    const int tid = threadIdx.x, j = tid % K, c = tid / K, team = c / kTeamRows, slot = c % kTeamRows;
    const int w = blockIdx.x * (8 / K) + team;
    const double pq = col_fold<K>(pq_part, pq_nparts, red);
    const bool act = !((fz >> j) & 1u) && pq != 0.0;
    const double alpha = act ? st->rho[it & 1][j] / pq : 0.0;
    if (blockIdx.x == 0 && tid < 64) {
        const unsigned mask = ~(unsigned)__ballot(act) & kFull;
        if (tid == 0) st->frozen_upd = mask;  // read by the direction launch of this iteration
    }
    double a0 = 0.0, a1 = 0.0;
    if (w < nteams) {
        for (int64_t row = (int64_t)w * kTeamRows + slot; row < nrows; row += (int64_t)nteams * kTeamRows) {
            const int64_t e = row * K + j;
            double rv = r[e];
            if (act) {
                const double t0 = alpha * p[e];
                x[e] = x[e] + t0;
                const double t1 = alpha * q[e];
                rv = rv - t1;
                r[e] = rv;
            }
            const double z = dinv ? dinv[row] * rv : rv;
            const double t2 = rv * z, t3 = rv * rv;
            a0 += t2;
            a1 += t3;
        }
    }
    const double s0 = team_sum<K>(a0, red, team);
    const double s1 = team_sum<K>(a1, red, team);
    if (slot == 0 && w < nteams) col_store_partials<K, true>(s0, s1, part, w, nteams);
}

// p_j = z_j + beta_j p_j for the columns that go on, beta_j = rho_new / rho_old from the folded partial sums of the
// update launch; workgroup 0 advances the state: rho, ||r||^2 and the count of the columns this iteration updated, the
// freeze mask of the next one (converged, or rho_new = 0).
template <int K>
__global__ __launch_bounds__(kBlock) void bcg_direction_kernel(int64_t nrows, int nteams, BcgState *st, int it,
                                                               const double *part, double rtol, double *__restrict__ p,
                                                               const double *__restrict__ r,
                                                               const double *__restrict__ dinv)
{
#pragma clang fp contract(off)
    __shared__ double red[32];
    constexpr unsigned kFull = (1u << K) - 1u;
    const unsigned fz = st->frozen[it & 1];
    if ((fz & kFull) == kFull) {
        // every column is frozen: nothing moves any more, but the slot the next iteration reads must say so too
        // (this launch writes the other slot only: the workgroups beside this one read slot it & 1)
        if (blockIdx.x == 0 && threadIdx.x == 0) st->frozen[(it + 1) & 1] = fz;
        return;
    }
    const int tid = threadIdx.x, j = tid % K, c = tid / K, team = c / kTeamRows, slot = c % kTeamRows;
    const int w = blockIdx.x * (8 / K) + team;
    const double rho_new = col_fold<K>(part, nteams, red);
    const double rr = col_fold<K>(part + (size_t)nteams * K, nteams, red);
    const bool act = !((st->frozen_upd >> j) & 1u);
    const double rho_old = st->rho[it & 1][j];
    const bool go_on = act && !(sqrt(rr) <= rtol * st->r0[j]) && rho_new != 0.0;
    const double beta = go_on ? rho_new / rho_old : 0.0;
    if (blockIdx.x == 0 && tid < 64) {
        const unsigned mask = ~(unsigned)__ballot(go_on) & kFull;
        if (tid < K) {
            st->rho[(it + 1) & 1][j] = act ? rho_new : rho_old;
            if (act) {
                st->rr[j] = rr;
                st->iters[j] = st->iters[j] + 1;
            }
        }
        if (tid == 0) {
            st->frozen[(it + 1) & 1] = mask;
            if (mask == kFull) st->stop_iter = 0;
        }
    }
    if (!go_on || w >= nteams) return;
    for (int64_t row = (int64_t)w * kTeamRows + slot; row < nrows; row += (int64_t)nteams * kTeamRows) {
        const int64_t e = row * K + j;
        const double rv = r[e];
        const double z = dinv ? dinv[row] * rv : rv;
        const double bp = beta * p[e];
        p[e] = z + bp;
    }
}

// 1 / a_ii per row (NaN where the row stores no diagonal entry); checked on the host
__global__ __launch_bounds__(kBlock) void bcg_dinv_kernel(CsrView A, double *__restrict__ dinv)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.nrows; i += stride) {
        double d = 0.0;
        bool found = false;
        for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
            if (A.col[k] == i) {
                d = A.val[k];
                found = true;
            }
        dinv[i] = found ? 1.0 / d : __builtin_nan("");
    }
}

static bool batch_k_ok(int k) { return k == 2 || k == 4 || k == 8; }

static int batch_spmm_grid(const CsrView &A) { return std::max(1, std::min(A.ntiles, kBatchGrid)); }

// teams of the vector launches: one per 32 rows up to kBatchGrid; a function of the number of rows alone
static int batch_teams(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kTeamRows - 1) / kTeamRows, kBatchGrid)); }

template <int K>
static void batch_spmm_launch_k(const CsrView &A, int mode, const BatchArgs &a, int grid, hipStream_t st)
{
    switch (mode) {
    case kBatchPlain: hipLaunchKernelGGL((batch_spmm_kernel<K, kBatchPlain>), dim3(grid), dim3(kBlock), 0, st, A, a); break;
    case kBatchDot: hipLaunchKernelGGL((batch_spmm_kernel<K, kBatchDot>), dim3(grid), dim3(kBlock), 0, st, A, a); break;
    case kBatchResidInit:
        hipLaunchKernelGGL((batch_spmm_kernel<K, kBatchResidInit>), dim3(grid), dim3(kBlock), 0, st, A, a);
        break;
    case kBatchResid: hipLaunchKernelGGL((batch_spmm_kernel<K, kBatchResid>), dim3(grid), dim3(kBlock), 0, st, A, a); break;
    default: hipLaunchKernelGGL((batch_spmm_kernel<K, kBatchResidNorm>), dim3(grid), dim3(kBlock), 0, st, A, a); break;
    }
}

// f(std::integral_constant<int, K>) for K = 2, 4, 8 (checked by the caller)
template <typename F>
static void batch_k_dispatch(int k, F &&f)
{
    if (k == 2)
        f(std::integral_constant<int, 2>());
    else if (k == 4)
        f(std::integral_constant<int, 4>());
    else
        f(std::integral_constant<int, 8>());
}

static void batch_spmm_launch(const CsrView &A, int k, int mode, const BatchArgs &a, int grid, hipStream_t st)
{
    batch_k_dispatch(k, [&](auto kc) { batch_spmm_launch_k<decltype(kc)::value>(A, mode, a, grid, st); });
}

}  // namespace schwz

using namespace schwz;

struct schwz_bcg {
    const schwz_csr *A = nullptr;
    int precond = 0, k = 0;
    int64_t n = 0;
    Dev<double> r, p, q, dinv;
    Dev<double> part;  // K kBatchGrid slots of p.q, then two banks of r.z and r.r
    Dev<double> norms;  // K: what schwz_bcg_residual folds
    StateMirror<BcgState> state;
    int gs = 0, nteams = 0;  // workgroups of the matrix launches and teams of the vector launches, both <= kBatchGrid
    bool solved = false;
};

static int bcg_build(schwz_bcg *s)
{
    const CsrView &A = s->A->v;
    const int64_t n = s->n;
    s->gs = batch_spmm_grid(A);
    s->nteams = batch_teams(n);
    int rc;
    for (Dev<double> *v : {&s->r, &s->p, &s->q})
        if ((rc = v->alloc((size_t)n * s->k, true))) return rc;
    if ((rc = s->part.alloc((size_t)3 * s->k * kBatchGrid, true)) || (rc = s->norms.alloc((size_t)s->k, true)) ||
        (rc = s->state.create()))
        return rc;
    if (s->precond == SCHWZ_PRECOND_JACOBI && n > 0) {
        if ((rc = s->dinv.alloc((size_t)n, true))) return rc;
        hipLaunchKernelGGL(bcg_dinv_kernel, dim3(grid_for(n)), dim3(kBlock), 0, 0, A, s->dinv);
        SCHWZ_HIP_TRY(hipGetLastError());
        std::vector<double> h((size_t)n);
        SCHWZ_HIP_TRY(hipMemcpy(h.data(), s->dinv, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i)
            if (!(h[(size_t)i] > 0.0) || !std::isfinite(h[(size_t)i])) {
                set_error("schwz_bcg_create: row " + std::to_string(i) +
                          " has no positive finite diagonal entry (Jacobi needs one)");
                return SCHWZ_ERR_NOT_SPD;
            }
    }
    SCHWZ_HIP_TRY(hipDeviceSynchronize());
    return SCHWZ_OK;
}

extern "C" {

int schwz_csr_spmm(const schwz_csr *A, int k, double alpha, const double *d_x, double beta, double *d_y,
                   schwz_stream stream)
{
    SCHWZ_REQUIRE(batch_k_ok(k), "schwz_csr_spmm: k must be 2, 4 or 8");
    SCHWZ_REQUIRE(A && d_x && d_y, "schwz_csr_spmm: null argument");
    if (A->v.nrows == 0) return SCHWZ_OK;
    BatchArgs a;
    a.alpha = alpha;
    a.beta = beta;
    a.x = d_x;
    a.y = d_y;
    batch_spmm_launch(A->v, k, kBatchPlain, a, batch_spmm_grid(A->v), (hipStream_t)stream);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_bcg_create(const schwz_csr *A, int precond, int k, schwz_bcg **out)
{
    // the argument checks come before the matrix is looked at (they need no device)
    SCHWZ_REQUIRE(out, "schwz_bcg_create: null output");
    *out = nullptr;
    SCHWZ_REQUIRE(batch_k_ok(k), "schwz_bcg_create: k must be 2, 4 or 8");
    SCHWZ_REQUIRE(precond >= SCHWZ_PRECOND_NONE && precond <= SCHWZ_PRECOND_ISAI, "schwz_bcg_create: unknown preconditioner");
    if (precond != SCHWZ_PRECOND_NONE && precond != SCHWZ_PRECOND_JACOBI) {
        set_error("schwz_bcg_create: the block CG exists without a preconditioner and with scalar Jacobi only");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    SCHWZ_REQUIRE(A, "schwz_bcg_create: null matrix");
    SCHWZ_REQUIRE(A->v.nrows == A->v.ncols, "schwz_bcg_create: matrix not square");
    schwz_bcg *s = new schwz_bcg();
    s->A = A;
    s->precond = precond;
    s->k = k;
    s->n = A->v.nrows;
    const int rc = bcg_build(s);
    if (rc) {
        schwz_bcg_destroy(s);
        return rc;
    }
    *out = s;
    return SCHWZ_OK;
}

void schwz_bcg_destroy(schwz_bcg *s) { delete s; }

int schwz_bcg_solve(schwz_bcg *s, const double *d_b, double *d_x, double rtol, int max_iters, unsigned frozen,
                    int *h_iters, double *h_resnorm, schwz_stream stream)
{
    SCHWZ_REQUIRE(s && d_b && d_x, "schwz_bcg_solve: null argument");
    SCHWZ_REQUIRE(max_iters >= 0, "schwz_bcg_solve: negative max_iters");
    SCHWZ_REQUIRE((frozen >> s->k) == 0, "schwz_bcg_solve: the frozen mask names a column >= k");
    hipStream_t st = (hipStream_t)stream;
    const int k = s->k;
    s->solved = true;
    if (s->n == 0) {
        for (int j = 0; j < k; ++j) {
            if (h_iters) h_iters[j] = 0;
            if (h_resnorm) h_resnorm[j] = 0.0;
        }
        return SCHWZ_OK;
    }
    const CsrView &A = s->A->v;
    const int gv = (s->nteams + 8 / k - 1) / (8 / k);  // workgroups of the vector launches: 8 / k teams each
    double *const pq_part = s->part, *const v_part = s->part + (size_t)k * kBatchGrid;
    BcgState *const dst = s->state.dev();
    // R = B - A X, P = M^-1 R, then the state from the folded r.z and r.r
    BatchArgs a;
    a.x = d_x;
    a.b = d_b;
    a.y = s->r;
    a.p = s->p;
    a.dinv = s->dinv;
    a.part = v_part;
    batch_spmm_launch(A, k, kBatchResidInit, a, s->gs, st);
    batch_k_dispatch(k, [&](auto kc) {
        hipLaunchKernelGGL((bcg_start_kernel<decltype(kc)::value>), dim3(1), dim3(kBlock), 0, st, dst, (const double *)v_part,
                           s->gs, rtol, frozen);
    });
    SCHWZ_HIP_TRY(hipGetLastError());
    BatchArgs d;
    d.x = s->p;
    d.y = s->q;
    d.part = pq_part;
    d.st = dst;
    auto iterate = [&](int it) {
        d.it = it;
        batch_spmm_launch(A, k, kBatchDot, d, s->gs, st);
        batch_k_dispatch(k, [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            hipLaunchKernelGGL((bcg_update_kernel<K>), dim3(gv), dim3(kBlock), 0, st, s->n, s->nteams, dst, it,
                               (const double *)pq_part, s->gs, d_x, (double *)s->r, (const double *)s->p,
                               (const double *)s->q, (const double *)s->dinv, v_part);
            hipLaunchKernelGGL((bcg_direction_kernel<K>), dim3(gv), dim3(kBlock), 0, st, s->n, s->nteams, dst, it,
                               (const double *)v_part, rtol, (double *)s->p, (const double *)s->r,
                               (const double *)s->dinv);
        });
    };
    if (!(rtol > 0.0)) {
        // fixed work: exactly max_iters iterations are launched; the host polls nothing
        for (int it = 0; it < max_iters; ++it) iterate(it);
        SCHWZ_HIP_TRY(hipGetLastError());
    } else {
        // growing chunks of launches and a poll of the pinned state copy one chunk behind, as in schwz_cheb_solve;
        // launches past the stop return at once
        ChunkSchedule chunks;
        int it = 0, rc;
        bool stopped = false;
        s->state.begin();
        while (it < max_iters && !stopped) {
            const int end = chunks.end(it, max_iters, true);
            for (; it < end; ++it) iterate(it);
            SCHWZ_HIP_TRY(hipGetLastError());
            if (it < max_iters) {
                if ((rc = s->state.poll(st, &stopped))) return rc;
                chunks.grow();
            }
        }
    }
    if (h_iters || h_resnorm) {
        if (const int rc = s->state.read(st)) return rc;
        for (int j = 0; j < k; ++j) {
            if (h_iters) h_iters[j] = s->state.host(0).iters[j];
            if (h_resnorm) h_resnorm[j] = std::sqrt(s->state.host(0).rr[j]);
        }
    }
    return SCHWZ_OK;
}

int schwz_bcg_last_stats(schwz_bcg *s, int *h_iters, double *h_resnorm)
{
    SCHWZ_REQUIRE(s && h_iters && h_resnorm, "schwz_bcg_last_stats: null argument");
    if (!s->solved || s->n == 0) {
        for (int j = 0; j < s->k; ++j) {
            h_iters[j] = 0;
            h_resnorm[j] = 0.0;
        }
        return SCHWZ_OK;
    }
    if (const int rc = s->state.read_blocking()) return rc;
    for (int j = 0; j < s->k; ++j) {
        h_iters[j] = s->state.host(0).iters[j];
        h_resnorm[j] = std::sqrt(s->state.host(0).rr[j]);
    }
    return SCHWZ_OK;
}

// per column the sum of (b - A x)^2 over the rows below row_limit, to the host (waits for `st`); R stored where d_r is
// given (then over all rows)
static int bcg_residual_impl(schwz_bcg *s, const double *d_b, const double *d_x, double *d_r, int64_t row_limit,
                             double *h_norm_sq, hipStream_t st)
{
    const int k = s->k;
    if (s->n == 0) {
        for (int j = 0; j < k; ++j) h_norm_sq[j] = 0.0;
        return SCHWZ_OK;
    }
    BatchArgs a;
    a.x = d_x;
    a.b = d_b;
    a.y = d_r;
    a.part = s->part + (size_t)k * kBatchGrid;
    a.row_limit = row_limit;
    batch_spmm_launch(s->A->v, k, d_r ? kBatchResid : kBatchResidNorm, a, s->gs, st);
    batch_k_dispatch(k, [&](auto kc) {
        hipLaunchKernelGGL((batch_fold_kernel<decltype(kc)::value>), dim3(1), dim3(kBlock), 0, st, (const double *)a.part,
                           s->gs, (double *)s->norms);
    });
    SCHWZ_HIP_TRY(hipGetLastError());
    SCHWZ_HIP_TRY(hipMemcpyAsync(h_norm_sq, s->norms, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    SCHWZ_HIP_TRY(hipStreamSynchronize(st));
    return SCHWZ_OK;
}

int schwz_bcg_residual(schwz_bcg *s, const double *d_b, const double *d_x, double *d_r, double *h_norm_sq,
                       schwz_stream stream)
{
    SCHWZ_REQUIRE(s && d_b && d_x && h_norm_sq, "schwz_bcg_residual: null argument");
    return bcg_residual_impl(s, d_b, d_x, d_r, INT64_MAX, h_norm_sq, (hipStream_t)stream);
}

}  // extern "C"

// ===========================================================================
// The steps of a RAS iteration on block vectors.  The block state of a subdomain -- x~ [interior | overlap | halo],
// b, b~ and y, k columns each, and a block CG on the local matrix -- is allocated by schwz_ras_batch_begin and is
// separate from the single-vector state: these entry points read the subdomain's matrix, interface rows and index
// lists and write nothing the single-vector entry points read.
// ===========================================================================

namespace schwz {

// into[e * k + j] = from[idx[e] * k + j] (PACK) or into[idx[e] * k + j] = from[e * k + j]: send and receive buffers are
// [neighbour][entry][column], the order of the index lists with the columns innermost
template <bool PACK>
__global__ __launch_bounds__(kBlock) void batch_halo_kernel(int64_t count, int k, const schwz_idx *__restrict__ idx,
                                                            const double *__restrict__ from, double *__restrict__ into)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < count * k; e += stride) {
        const int64_t at = (int64_t)idx[e / k] * k + e % k;
        if (PACK)
            into[e] = from[at];
        else
            into[at] = from[e];
    }
}

// b~ = b - A_Gamma x~ on the overlap rows, a lane per (row, column), the row sum in CSR order
__global__ __launch_bounds__(kBlock) void batch_interface_kernel(int64_t nrows, int64_t row0, int k,
                                                                 const schwz_idx *__restrict__ rp,
                                                                 const schwz_idx *__restrict__ col,
                                                                 const double *__restrict__ val, const double *__restrict__ x,
                                                                 const double *__restrict__ b, double *__restrict__ bt)
{
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nrows * k; e += stride) {
        const int64_t i = e / k;
        const int j = (int)(e % k);
        double s = 0.0;
        for (int q = rp[i]; q < rp[i + 1]; ++q) {
            const double pv = val[q] * x[(int64_t)col[q] * k + j];
            s += pv;
        }
        bt[(row0 + i) * k + j] = b[(row0 + i) * k + j] - s;
    }
}

// x~[interior] = y[interior] in the columns the mask does not name
__global__ __launch_bounds__(kBlock) void batch_restrict_kernel(int64_t count, int k, unsigned mask,
                                                                const double *__restrict__ y, double *__restrict__ x)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < count; e += stride)
        if (!((mask >> (e % k)) & 1u)) x[e] = y[e];
}

}  // namespace schwz

#define REQUIRE_BATCH(sd, name)                                                 \
    SCHWZ_REQUIRE((sd) && (sd)->dev, name ": subdomain is not on the device"); \
    SCHWZ_REQUIRE((sd)->dev->batch, name ": the subdomain has no block state (schwz_ras_batch_begin)")

extern "C" {

int schwz_ras_batch_begin(schwz_subdomain *sd, int k)
{
    SCHWZ_REQUIRE(batch_k_ok(k), "schwz_ras_batch_begin: k must be 2, 4 or 8");
    SCHWZ_REQUIRE(sd && sd->dev, "schwz_ras_batch_begin: subdomain is not on the device");
    const schwz_solver_options &o = sd->opt;
    const bool jacobi = o.precond == SCHWZ_PRECOND_JACOBI || (o.precond == SCHWZ_PRECOND_BLOCK_JACOBI && o.precond_block_size <= 1);
    if (o.local_solver != SCHWZ_SOLVER_ITERATIVE || o.non_symmetric || sd->dev->gmres || sd->dev->bicg ||
        !(jacobi || o.precond == SCHWZ_PRECOND_NONE) || o.par_ilu_sweeps || o.trisolve_sweeps ||
        sd->precision != SCHWZ_PRECISION_F64 || sd->sym_solver != SCHWZ_SYM_CG || sd->dev->coarse) {
        set_error("schwz_ras_batch_begin: the block path exists for the fp64 CG local solve of a symmetric matrix, without a "
                  "preconditioner or with scalar Jacobi, on one level");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    if (sd->dev->batch && sd->dev->batch->k != k) {
        delete sd->dev->batch;
        sd->dev->batch = nullptr;
    }
    const int64_t n = sd->local_size_x, nx = n + sd->halo_size;
    if (!sd->dev->batch) {
        schwz_ras_batch *b = new schwz_ras_batch();
        b->k = k;
        int rc;
        if ((rc = schwz_bcg_create(sd->dev->A, jacobi ? SCHWZ_PRECOND_JACOBI : SCHWZ_PRECOND_NONE, k, &b->cg)) ||
            (rc = b->x.alloc((size_t)nx * k, true)) || (rc = b->rhs.alloc((size_t)n * k, true)) ||
            (rc = b->bt.alloc((size_t)n * k, true)) || (rc = b->y.alloc((size_t)n * k, true))) {
            delete b;
            return rc;
        }
        SCHWZ_HIP_TRY(hipDeviceSynchronize());
        sd->dev->batch = b;
    }
    return SCHWZ_OK;
}

int schwz_ras_batch_end(schwz_subdomain *sd)
{
    SCHWZ_REQUIRE(sd, "schwz_ras_batch_end: null subdomain");
    if (!sd->dev) return SCHWZ_OK;
    delete sd->dev->batch;
    sd->dev->batch = nullptr;
    return SCHWZ_OK;
}

int schwz_ras_batch_rhs_set(schwz_subdomain *sd, const double *h_rhs, schwz_stream stream)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_rhs_set");
    SCHWZ_REQUIRE(h_rhs || sd->local_size_x == 0, "schwz_ras_batch_rhs_set: null right-hand side");
    schwz_ras_batch *b = sd->dev->batch;
    hipStream_t st = (hipStream_t)stream;
    const size_t nk = (size_t)sd->local_size_x * b->k, nxk = (size_t)(sd->local_size_x + sd->halo_size) * b->k;
    // the state a fresh upload leaves: x~ and y zero, b~ = b
    if (nxk) SCHWZ_HIP_TRY(hipMemsetAsync(b->x, 0, nxk * sizeof(double), st));
    if (nk) {
        SCHWZ_HIP_TRY(hipMemsetAsync(b->y, 0, nk * sizeof(double), st));
        SCHWZ_HIP_TRY(hipMemcpyAsync(b->rhs, h_rhs, nk * sizeof(double), hipMemcpyHostToDevice, st));
        const int rc = launch_copy((int64_t)nk, b->rhs, b->bt, st);
        if (rc) return rc;
    }
    SCHWZ_HIP_TRY(hipStreamSynchronize(st));  // the host array is the caller's again
    return SCHWZ_OK;
}

int schwz_ras_batch_pack(schwz_subdomain *sd, double *d_send, schwz_stream stream)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_pack");
    if (sd->num_send == 0) return SCHWZ_OK;
    SCHWZ_REQUIRE(d_send, "schwz_ras_batch_pack: null send buffer");
    const int k = sd->dev->batch->k;
    hipLaunchKernelGGL(batch_halo_kernel<true>, dim3(grid_for(sd->num_send * k)), dim3(kBlock), 0, (hipStream_t)stream,
                       sd->num_send, k, (const schwz_idx *)sd->dev->d_put_idx, (const double *)sd->dev->batch->x, d_send);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_ras_batch_unpack(schwz_subdomain *sd, const double *d_recv, schwz_stream stream)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_unpack");
    if (sd->num_recv == 0) return SCHWZ_OK;
    SCHWZ_REQUIRE(d_recv, "schwz_ras_batch_unpack: null recv buffer");
    const int k = sd->dev->batch->k;
    hipLaunchKernelGGL(batch_halo_kernel<false>, dim3(grid_for(sd->num_recv * k)), dim3(kBlock), 0, (hipStream_t)stream,
                       sd->num_recv, k, (const schwz_idx *)sd->dev->d_get_idx, d_recv, (double *)sd->dev->batch->x);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_ras_batch_update_boundary(schwz_subdomain *sd, schwz_stream stream)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_update_boundary");
    // as schwz_ras_update_boundary: rows < local_size have no interface entries, b~ = b there
    if (sd->P <= 1 || sd->nnz_interface == 0 || sd->overlap_size == 0) return SCHWZ_OK;
    schwz_ras_batch *b = sd->dev->batch;
    hipLaunchKernelGGL(batch_interface_kernel, dim3(grid_for(sd->overlap_size * b->k)), dim3(kBlock), 0, (hipStream_t)stream,
                       sd->overlap_size, sd->local_size, b->k, (const schwz_idx *)sd->dev->d_i_rp, (const schwz_idx *)sd->dev->d_i_col,
                       (const double *)sd->dev->d_i_val, (const double *)b->x, (const double *)b->rhs, (double *)b->bt);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_ras_batch_local_residual(schwz_subdomain *sd, double *h_resnorm, schwz_stream stream)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_local_residual");
    SCHWZ_REQUIRE(h_resnorm, "schwz_ras_batch_local_residual: null output");
    schwz_ras_batch *b = sd->dev->batch;
    const int rc = bcg_residual_impl(b->cg, b->bt, b->x, nullptr, INT64_MAX, h_resnorm, (hipStream_t)stream);
    if (rc) return rc;
    for (int j = 0; j < b->k; ++j) h_resnorm[j] = std::sqrt(h_resnorm[j]);
    return SCHWZ_OK;
}

int schwz_ras_batch_local_solve(schwz_subdomain *sd, unsigned frozen, int *h_inner_iters, schwz_stream stream)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_local_solve");
    schwz_ras_batch *b = sd->dev->batch;
    const int maxit = sd->opt.local_max_iters == -1 ? (int)sd->local_size_x : sd->opt.local_max_iters;
    return schwz_bcg_solve(b->cg, b->bt, b->y, sd->opt.local_tol, maxit, frozen, h_inner_iters, nullptr, stream);
}

int schwz_ras_batch_restrict(schwz_subdomain *sd, unsigned frozen, schwz_stream stream)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_restrict");
    schwz_ras_batch *b = sd->dev->batch;
    SCHWZ_REQUIRE((frozen >> b->k) == 0, "schwz_ras_batch_restrict: the mask names a column >= k");
    const int64_t count = sd->local_size * b->k;
    if (count == 0) return SCHWZ_OK;
    hipLaunchKernelGGL(batch_restrict_kernel, dim3(grid_for(count)), dim3(kBlock), 0, (hipStream_t)stream, count, b->k, frozen,
                       (const double *)b->y, (double *)b->x);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_ras_batch_vector(schwz_subdomain *sd, int which, double **d_ptr, int64_t *len)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_vector");
    SCHWZ_REQUIRE(d_ptr && len, "schwz_ras_batch_vector: null output");
    SCHWZ_REQUIRE(which >= 0 && which <= 3, "schwz_ras_batch_vector: which must be 0 (x~), 1 (b~), 2 (y) or 3 (b)");
    schwz_ras_batch *b = sd->dev->batch;
    const int64_t n = sd->local_size_x * b->k;
    *d_ptr = which == 0 ? b->x : which == 1 ? b->bt : which == 2 ? b->y : b->rhs;
    *len = which == 0 ? n + sd->halo_size * b->k : n;
    return SCHWZ_OK;
}

int schwz_ras_batch_get_interior(schwz_subdomain *sd, double *h_out, schwz_stream stream)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_get_interior");
    SCHWZ_REQUIRE(h_out || sd->local_size == 0, "schwz_ras_batch_get_interior: null output");
    if (sd->local_size == 0) return SCHWZ_OK;
    SCHWZ_HIP_TRY(hipMemcpyAsync(h_out, sd->dev->batch->x, (size_t)sd->local_size * sd->dev->batch->k * sizeof(double),
                                 hipMemcpyDeviceToHost, (hipStream_t)stream));
    SCHWZ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return SCHWZ_OK;
}

int schwz_ras_batch_true_residual_sq(schwz_subdomain *sd, double *h_out, schwz_stream stream)
{
    REQUIRE_BATCH(sd, "schwz_ras_batch_true_residual_sq");
    SCHWZ_REQUIRE(h_out, "schwz_ras_batch_true_residual_sq: null output");
    schwz_ras_batch *b = sd->dev->batch;
    return bcg_residual_impl(b->cg, b->rhs, b->x, nullptr, sd->local_size, h_out, (hipStream_t)stream);
}

}  // extern "C"
