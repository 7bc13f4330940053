// Fine-grained GPU ILU: ParILU factors (Chow & Patel's fixed-point sweeps, the factorization the
// reference builds as gko::factorization::ParIlu, source/solve.cpp:506-532) and triangular solves by
// Jacobi sweeps (the truncated Neumann series of each factor).  Neither kernel waits on another
// workgroup: a sweep is one launch that reads the previous iterate and writes the next one.
//
// ParILU.  The factors live on the ILU(0) pattern of A: L unit lower with its 1 stored last in each
// row, U upper with its diagonal first (the layout of schwz_ilu0 / schwz_trs_create).  Start: L0 = the
// strict lower part of A with a unit diagonal, U0 = the upper part of A.  One synchronous sweep:
//     l_ij = (a_ij - sum_{k<j} l_ik u_kj) / u_jj      (i > j)
//     u_ij =  a_ij - sum_{k<i} l_ik u_kj              (i <= j)
// with every l, u on the right taken from the previous sweep.  After as many sweeps as the longest
// dependency chain among the entries the iterate is the exact ILU(0).  A symbolic pass on the host
// (once per pattern) lists for every entry of A the (L index, U index) pairs of its sum, k ascending;
// a sweep is then a regular gather over that list.
//
// Jacobi-sweep solves.  For T = D + T_s: x_0 = D^-1 b, x_{m+1} = D^-1 (b - T_s x_m), k times per factor:
// x_k = sum_{m=0..k} (-D^-1 T_s)^m D^-1 b, exact once k >= levels - 1.  One lane per row over the strict
// part in CSR; the D^-1 b start of a factor is formed inside its first pass (no launch of its own).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "schwz_internal.hpp"

namespace schwz {

// first iterate: L0 = strict lower part of A, U0 = upper part (dst >= 0: U index, < 0: L index -(dst+1))
__global__ __launch_bounds__(kBlock) void parilu_init_kernel(int64_t nnz, const double *__restrict__ a,
                                                             const int2 *__restrict__ dst, double *__restrict__ lv,
                                                             double *__restrict__ uv)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += stride) {
        const int d = dst[e].x;
        if (d >= 0)
            uv[d] = a[e];
        else
            lv[-(d + 1)] = a[e];
    }
}

// the unit diagonal of L (last entry of each row), in both buffers
__global__ __launch_bounds__(kBlock) void parilu_unit_kernel(int64_t n, const schwz_idx *__restrict__ l_rp,
                                                             double *__restrict__ l0, double *__restrict__ l1)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const schwz_idx j = l_rp[i + 1] - 1;
        l0[j] = 1.0;
        l1[j] = 1.0;
    }
}

// one synchronous sweep: (lo, uo) -> (ln, un).  dst[e] = {target index, U index of the pivot u_jj (L entries)}
__global__ __launch_bounds__(kBlock) void parilu_sweep_kernel(int64_t nnz, const double *__restrict__ a,
                                                              const int2 *__restrict__ dst,
                                                              const schwz_idx *__restrict__ pp,
                                                              const int2 *__restrict__ pairs,
                                                              const double *__restrict__ lo,
                                                              const double *__restrict__ uo, double *__restrict__ ln,
                                                              double *__restrict__ un)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += stride) {
        double s = a[e];
        const schwz_idx p1 = pp[e + 1];
        for (schwz_idx p = pp[e]; p < p1; ++p) {
            const int2 q = pairs[p];
            s -= lo[q.x] * uo[q.y];
        }
        const int2 d = dst[e];
        if (d.x >= 0)
            un[d.x] = s;
        else
            ln[-(d.x + 1)] = s / uo[d.y];
    }
}

// breakdown check: bad = 1 when some u_ii is zero or not finite (plain vector store; racing writers store
// the same value)
__global__ __launch_bounds__(kBlock) void parilu_pivot_kernel(int64_t n, const schwz_idx *__restrict__ u_rp,
                                                              const double *__restrict__ uv, int *__restrict__ bad)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double d = uv[u_rp[i]];
        if (!(d != 0.0 && std::isfinite(d))) *bad = 1;
    }
}

// one Jacobi pass of a triangular solve: xn[i] = dinv[i] * (b[i] - sum_j t_ij xo[j]) over the strict part.
// FIRST: xo is the start D^-1 b0 formed on the fly from b0 = xo_src and dinv_src.
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void trs_jacobi_kernel(int64_t n, const schwz_idx *__restrict__ rp,
                                                            const schwz_idx *__restrict__ col,
                                                            const double *__restrict__ val,
                                                            const double *__restrict__ dinv,
                                                            const double *__restrict__ b,
                                                            const double *__restrict__ xo,
                                                            const double *__restrict__ dinv_src,
                                                            double *__restrict__ xn)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double s = b[i];
        const schwz_idx j1 = rp[i + 1];
        for (schwz_idx j = rp[i]; j < j1; ++j) {
            const schwz_idx c = col[j];
            const double x = FIRST ? dinv_src[c] * xo[c] : xo[c];
            s -= val[j] * x;
        }
        xn[i] = dinv[i] * s;
    }
}

// y = U^-1 L^-1 b by `sweeps` Jacobi passes per factor (schwz_trs in sweep mode)
int trs_sweeps_solve(schwz_trs *t, const double *b, double *y, hipStream_t st)
{
    const int64_t n = t->n;
    const int k = t->sweeps;
    const int g = grid_for(n);
    double *w[2] = {t->w0, t->w1};
    // L: pass m (1..k) writes w[(m-1) & 1]
    for (int m = 1; m <= k; ++m) {
        double *out = w[(m - 1) & 1];
        if (m == 1)
            hipLaunchKernelGGL(trs_jacobi_kernel<true>, dim3(g), dim3(kBlock), 0, st, n, t->js_l_rp, t->js_l_col,
                               t->js_l_val, t->js_l_dinv, b, b, t->js_l_dinv, out);
        else
            hipLaunchKernelGGL(trs_jacobi_kernel<false>, dim3(g), dim3(kBlock), 0, st, n, t->js_l_rp, t->js_l_col,
                               t->js_l_val, t->js_l_dinv, b, w[m & 1], (const double *)nullptr, out);
    }
    // U with r = L's result as its right-hand side: the last pass writes y, the others alternate between
    // the two free buffers
    const double *r = w[(k - 1) & 1];
    double *free_buf[2] = {t->w2, w[k & 1]};
    const double *prev = r;
    for (int m = 1; m <= k; ++m) {
        double *out = m == k ? y : free_buf[(m - 1) & 1];
        if (m == 1)
            hipLaunchKernelGGL(trs_jacobi_kernel<true>, dim3(g), dim3(kBlock), 0, st, n, t->js_u_rp, t->js_u_col,
                               t->js_u_val, t->js_u_dinv, r, r, t->js_u_dinv, out);
        else
            hipLaunchKernelGGL(trs_jacobi_kernel<false>, dim3(g), dim3(kBlock), 0, st, n, t->js_u_rp, t->js_u_col,
                               t->js_u_val, t->js_u_dinv, r, prev, (const double *)nullptr, out);
        prev = out;
    }
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

// ParILU symbolic pass + sweeps.  h_rp / h_col: the pattern of A on the host (columns sorted, diagonal
// present); d_val: A's values in HBM.  Outputs: the L / U patterns (malloc'd host arrays) and their values
// in HBM.
static int parilu_run(int64_t n, const schwz_idx *h_rp, const schwz_idx *h_col, const double *d_val, int sweeps,
                      schwz_idx **l_rp_o, schwz_idx **l_col_o, Dev<double> *d_l_val_o, schwz_idx **u_rp_o,
                      schwz_idx **u_col_o, Dev<double> *d_u_val_o)
{
    SCHWZ_REQUIRE(sweeps >= 1, "schwz_parilu: sweeps must be >= 1");
    SCHWZ_REQUIRE(n >= 0 && n < INT32_MAX, "schwz_parilu: bad size");
    const int64_t nnz = h_rp[n];
    SCHWZ_REQUIRE(nnz < INT32_MAX - n, "schwz_parilu: more than 2^31-1 factor entries");
    StageTimer timer_sym("parilu: symbolic pass (pattern, pair lists)");
    // L / U row pointers; per entry of A its target index
    std::vector<schwz_idx> l_rp((size_t)n + 1, 0), u_rp((size_t)n + 1, 0);
    std::vector<schwz_idx> nlow((size_t)n);
    std::vector<int> bad_row((size_t)setup_threads(), -1);
    parallel_blocks(n, 4096, [&](int t, int, int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            schwz_idx lo = 0;
            bool diag = false;
            for (schwz_idx j = h_rp[i]; j < h_rp[i + 1]; ++j) {
                if ((j > h_rp[i] && h_col[j - 1] >= h_col[j]) || h_col[j] < 0 || h_col[j] >= n) {
                    bad_row[(size_t)t] = 0;
                    return;
                }
                if (h_col[j] < i) ++lo;
                if (h_col[j] == i) diag = true;
            }
            if (!diag) {
                bad_row[(size_t)t] = 1;
                return;
            }
            nlow[(size_t)i] = lo;
        }
    });
    for (int b : bad_row) {
        SCHWZ_REQUIRE(b != 0, "schwz_parilu: columns must be sorted, unique and inside the matrix");
        SCHWZ_REQUIRE(b != 1, "schwz_parilu: structurally zero diagonal");
    }
    for (int64_t i = 0; i < n; ++i) {
        l_rp[(size_t)i + 1] = l_rp[(size_t)i] + nlow[(size_t)i] + 1;
        u_rp[(size_t)i + 1] = u_rp[(size_t)i] + (h_rp[i + 1] - h_rp[i] - nlow[(size_t)i]);
    }
    std::vector<schwz_idx> l_col((size_t)l_rp[(size_t)n]), u_col((size_t)u_rp[(size_t)n]);
    std::vector<int2> dst((size_t)nnz);
    // index of an entry of A in L or U
    auto target = [&](int64_t i, schwz_idx j) -> schwz_idx {
        const schwz_idx off = j - h_rp[i];
        return off < nlow[(size_t)i] ? l_rp[(size_t)i] + off : u_rp[(size_t)i] + off - nlow[(size_t)i];
    };
    std::vector<schwz_idx> pp((size_t)nnz + 1, 0);
    // pass 1: targets, factor columns and the pair count of every entry; pass 2: the pairs.  Row i's pairs
    // come from its lower entries (i, k), k ascending, times the U row k beyond its diagonal.
    // entries of row i matched against U row k beyond its diagonal: both column lists are sorted, so a merge
    auto row_pairs = [&](int64_t i, bool fill, int2 *pairs) {
        const schwz_idx i0 = h_rp[i], i1 = h_rp[i + 1];
        for (schwz_idx kk = i0; kk < i0 + nlow[(size_t)i]; ++kk) {
            const schwz_idx k = h_col[kk];
            const schwz_idx lidx = l_rp[(size_t)i] + (kk - i0);
            schwz_idx e = kk + 1;
            for (schwz_idx q = h_rp[k] + nlow[(size_t)k] + 1; q < h_rp[k + 1] && e < i1; ++q) {
                while (e < i1 && h_col[e] < h_col[q]) ++e;
                if (e == i1 || h_col[e] != h_col[q]) continue;
                if (fill)
                    pairs[pp[(size_t)e + 1]++] = make_int2(lidx, u_rp[(size_t)k] + (q - h_rp[k] - nlow[(size_t)k]));
                else
                    ++pp[(size_t)e + 1];
            }
        }
    };
    parallel_blocks(n, 4096, [&](int, int, int64_t r0, int64_t r1) {
        for (int64_t i = r0; i < r1; ++i) {
            for (schwz_idx j = h_rp[i]; j < h_rp[i + 1]; ++j) {
                const schwz_idx c = h_col[j], d = target(i, j);
                if (c < i) {
                    l_col[(size_t)d] = c;
                    dst[(size_t)j] = make_int2(-(d + 1), u_rp[(size_t)c]);
                } else {
                    u_col[(size_t)d] = c;
                    dst[(size_t)j] = make_int2(d, 0);
                }
            }
            l_col[(size_t)l_rp[(size_t)i + 1] - 1] = (schwz_idx)i;
            row_pairs(i, false, nullptr);
        }
    });
    int64_t total = 0;
    for (int64_t e = 0; e < nnz; ++e) {
        total += pp[(size_t)e + 1];
        SCHWZ_REQUIRE(total < INT32_MAX, "schwz_parilu: more than 2^31-1 products per sweep");
        pp[(size_t)e + 1] = (schwz_idx)total;
    }
    const int64_t npairs = total;
    std::vector<int2> pairs((size_t)(npairs ? npairs : 1));
    // pass 2 advances pp[e + 1] from the start of entry e: shift by one first
    std::memmove(pp.data() + 1, pp.data(), (size_t)nnz * sizeof(schwz_idx));
    parallel_blocks(n, 4096, [&](int, int, int64_t r0, int64_t r1) {
        for (int64_t i = r0; i < r1; ++i) row_pairs(i, true, pairs.data());
    });
    timer_sym.stop();
    StageTimer timer_sw("parilu: upload + sweeps + pivot check");
    const int64_t lnz = l_rp[(size_t)n], unz = u_rp[(size_t)n];
    Dev<int2> d_dst, d_pairs;
    Dev<schwz_idx> d_pp, d_lrp, d_urp;
    Dev<double> lv[2], uv[2];
    Dev<int> d_bad;
    int rc;
    if ((rc = d_dst.put(dst)) || (rc = d_pp.put(pp)) || (rc = d_pairs.put(pairs.data(), (size_t)npairs)) ||
        (rc = d_lrp.put(l_rp)) || (rc = d_urp.put(u_rp)))
        return rc;
    for (int b = 0; b < 2 && !rc; ++b)
        if (!(rc = lv[b].alloc((size_t)(lnz ? lnz : 1)))) rc = uv[b].alloc((size_t)(unz ? unz : 1));
    if (!rc) rc = d_bad.alloc(1);
    if (rc) {
        (void)hipGetLastError();
        set_error("schwz_parilu: out of device memory");
        return rc;
    }
    const int g_e = grid_for(nnz), g_n = grid_for(n);
    const hipStream_t st = nullptr;
    hipLaunchKernelGGL(parilu_init_kernel, dim3(g_e), dim3(kBlock), 0, st, nnz, d_val, (const int2 *)d_dst,
                       (double *)lv[0], (double *)uv[0]);
    hipLaunchKernelGGL(parilu_unit_kernel, dim3(g_n), dim3(kBlock), 0, st, n, (const schwz_idx *)d_lrp, (double *)lv[0],
                       (double *)lv[1]);
    for (int s = 0; s < sweeps; ++s) {
        const int o = s & 1;
        hipLaunchKernelGGL(parilu_sweep_kernel, dim3(g_e), dim3(kBlock), 0, st, nnz, d_val, (const int2 *)d_dst,
                           (const schwz_idx *)d_pp, (const int2 *)d_pairs, (const double *)lv[o],
                           (const double *)uv[o], (double *)lv[o ^ 1], (double *)uv[o ^ 1]);
    }
    const int fin = sweeps & 1;
    int bad = 0;
    hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(int), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(parilu_pivot_kernel, dim3(g_n), dim3(kBlock), 0, st, n, (const schwz_idx *)d_urp,
                           (const double *)uv[fin], (int *)d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        set_error(std::string("schwz_parilu: ") + hipGetErrorString(e));
        return SCHWZ_ERR_HIP;
    }
    if (bad) {
        set_error("schwz_parilu: zero or non-finite pivot after " + std::to_string(sweeps) + " ParILU sweep" +
                  (sweeps == 1 ? "" : "s"));
        return SCHWZ_ERR_NOT_SPD;
    }
    auto to_malloc = [](const std::vector<schwz_idx> &v) {
        schwz_idx *p = (schwz_idx *)std::malloc(sizeof(schwz_idx) * (v.size() ? v.size() : 1));
        if (p && !v.empty()) std::memcpy(p, v.data(), sizeof(schwz_idx) * v.size());
        return p;
    };
    *l_rp_o = to_malloc(l_rp);
    *l_col_o = to_malloc(l_col);
    *u_rp_o = to_malloc(u_rp);
    *u_col_o = to_malloc(u_col);
    if (!*l_rp_o || !*l_col_o || !*u_rp_o || !*u_col_o) {
        for (void *p : {(void *)*l_rp_o, (void *)*l_col_o, (void *)*u_rp_o, (void *)*u_col_o}) std::free(p);
        set_error("schwz_parilu: out of host memory");
        return SCHWZ_ERR_INVALID;
    }
    *d_l_val_o = std::move(lv[fin]);
    *d_u_val_o = std::move(uv[fin]);
    return SCHWZ_OK;
}

// the factors of parilu_run with their values copied to the host (malloc'd): what the exact-solve plan,
// the sweep solves and the ISAI construction take
int parilu_host_factors(int64_t n, const schwz_idx *h_rp, const schwz_idx *h_col, const double *d_val, int sweeps,
                        schwz_idx **l_rp, schwz_idx **l_col, double **l_val, schwz_idx **u_rp, schwz_idx **u_col,
                        double **u_val)
{
    Dev<double> dl, du;
    int rc = parilu_run(n, h_rp, h_col, d_val, sweeps, l_rp, l_col, &dl, u_rp, u_col, &du);
    if (rc) return rc;
    const size_t lnz = (size_t)(*l_rp)[n], unz = (size_t)(*u_rp)[n];
    *l_val = (double *)std::malloc(sizeof(double) * (lnz ? lnz : 1));
    *u_val = (double *)std::malloc(sizeof(double) * (unz ? unz : 1));
    hipError_t e = hipSuccess;
    if (*l_val && *u_val) {
        e = hipMemcpy(*l_val, dl, sizeof(double) * lnz, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(*u_val, du, sizeof(double) * unz, hipMemcpyDeviceToHost);
    }
    if (!*l_val || !*u_val || e != hipSuccess) {
        for (void *p : {(void *)*l_rp, (void *)*l_col, (void *)*l_val, (void *)*u_rp, (void *)*u_col, (void *)*u_val})
            std::free(p);
        set_error(e != hipSuccess ? std::string("schwz_parilu: ") + hipGetErrorString(e)
                                  : std::string("schwz_parilu: out of host memory"));
        return e != hipSuccess ? SCHWZ_ERR_HIP : SCHWZ_ERR_INVALID;
    }
    return SCHWZ_OK;
}

}  // namespace schwz

using namespace schwz;

extern "C" {

int schwz_parilu(const schwz_csr *A, int sweeps, schwz_idx **l_rp, schwz_idx **l_col, double **d_l_val,
                 schwz_idx **u_rp, schwz_idx **u_col, double **d_u_val)
{
    SCHWZ_REQUIRE(A && l_rp && l_col && d_l_val && u_rp && u_col && d_u_val, "schwz_parilu: null argument");
    SCHWZ_REQUIRE(A->v.nrows == A->v.ncols, "schwz_parilu: matrix not square");
    const int64_t n = A->v.nrows;
    // the pattern (not the values) comes back for the symbolic pass
    std::vector<schwz_idx> rp((size_t)n + 1), col((size_t)A->v.nnz);
    SCHWZ_HIP_TRY(hipMemcpy(rp.data(), A->v.rp, rp.size() * sizeof(schwz_idx), hipMemcpyDeviceToHost));
    if (!col.empty())
        SCHWZ_HIP_TRY(hipMemcpy(col.data(), A->v.col, col.size() * sizeof(schwz_idx), hipMemcpyDeviceToHost));
    Dev<double> dl, du;
    if (int rc = parilu_run(n, rp.data(), col.data(), A->v.val, sweeps, l_rp, l_col, &dl, u_rp, u_col, &du)) return rc;
    // success only: the values leave their owners for the caller (schwz_device_free)
    *d_l_val = (double *)dl.release();
    *d_u_val = (double *)du.release();
    return SCHWZ_OK;
}

int schwz_parilu_host(int64_t n, const schwz_idx *h_rp, const schwz_idx *h_col, const double *h_val, int sweeps,
                      schwz_idx **l_rp, schwz_idx **l_col, double **l_val, schwz_idx **u_rp, schwz_idx **u_col,
                      double **u_val)
{
    SCHWZ_REQUIRE(h_rp && l_rp && l_col && l_val && u_rp && u_col && u_val && n >= 0, "schwz_parilu_host: bad arguments");
    SCHWZ_REQUIRE(h_rp[0] == 0 && h_rp[n] >= 0 && (h_rp[n] == 0 || (h_col && h_val)), "schwz_parilu_host: bad arguments");
    Dev<double> d_val;
    if (int rc = d_val.put(h_val, (size_t)h_rp[n])) return rc;
    return parilu_host_factors(n, h_rp, h_col, d_val, sweeps, l_rp, l_col, l_val, u_rp, u_col, u_val);
}

void schwz_device_free(void *d_ptr) { (void)hipFree(d_ptr); }

int schwz_trs_create_sweeps(int64_t n, const schwz_idx *l_rp, const schwz_idx *l_col, const double *l_val,
                            const schwz_idx *u_rp, const schwz_idx *u_col, const double *u_val, int sweeps,
                            schwz_trs **out)
{
    SCHWZ_REQUIRE(out && n >= 0 && n < INT32_MAX && l_rp && u_rp, "schwz_trs_create_sweeps: bad arguments");
    SCHWZ_REQUIRE(sweeps >= 1, "schwz_trs_create_sweeps: sweeps must be >= 1");
    for (int64_t i = 0; i < n; ++i) {
        SCHWZ_REQUIRE(l_rp[i + 1] > l_rp[i] && l_col[l_rp[i + 1] - 1] == i,
                      "schwz_trs_create_sweeps: L must hold its diagonal last in each row");
        SCHWZ_REQUIRE(u_rp[i + 1] > u_rp[i] && u_col[u_rp[i]] == i,
                      "schwz_trs_create_sweeps: U must hold its diagonal first in each row");
        for (schwz_idx j = l_rp[i]; j < l_rp[i + 1] - 1; ++j)
            SCHWZ_REQUIRE(l_col[j] >= 0 && l_col[j] < i, "schwz_trs_create_sweeps: L is not lower triangular");
        for (schwz_idx j = u_rp[i] + 1; j < u_rp[i + 1]; ++j)
            SCHWZ_REQUIRE(u_col[j] > i && u_col[j] < n, "schwz_trs_create_sweeps: U is not upper triangular");
        SCHWZ_REQUIRE(l_val[l_rp[i + 1] - 1] != 0.0 && u_val[u_rp[i]] != 0.0,
                      "schwz_trs_create_sweeps: zero diagonal entry");
    }
    // strict parts in CSR + reciprocal diagonals
    std::vector<schwz_idx> lrp((size_t)n + 1, 0), urp((size_t)n + 1, 0), lcol, ucol;
    std::vector<double> lval, uval, ldi((size_t)n), udi((size_t)n);
    lcol.reserve((size_t)(l_rp[n] - n));
    lval.reserve((size_t)(l_rp[n] - n));
    ucol.reserve((size_t)(u_rp[n] - n));
    uval.reserve((size_t)(u_rp[n] - n));
    for (int64_t i = 0; i < n; ++i) {
        for (schwz_idx j = l_rp[i]; j < l_rp[i + 1] - 1; ++j) {
            lcol.push_back(l_col[j]);
            lval.push_back(l_val[j]);
        }
        for (schwz_idx j = u_rp[i] + 1; j < u_rp[i + 1]; ++j) {
            ucol.push_back(u_col[j]);
            uval.push_back(u_val[j]);
        }
        lrp[(size_t)i + 1] = (schwz_idx)lcol.size();
        urp[(size_t)i + 1] = (schwz_idx)ucol.size();
        ldi[(size_t)i] = 1.0 / l_val[l_rp[i + 1] - 1];
        udi[(size_t)i] = 1.0 / u_val[u_rp[i]];
    }
    schwz_trs *t = new schwz_trs();
    t->n = n;
    t->sweeps = sweeps;
    std::unique_ptr<schwz_trs> own(t);
    int rc;
    if ((rc = t->js_l_rp.put(lrp)) || (rc = t->js_l_col.put(lcol)) || (rc = t->js_l_val.put(lval)) ||
        (rc = t->js_l_dinv.put(ldi)) || (rc = t->js_u_rp.put(urp)) || (rc = t->js_u_col.put(ucol)) ||
        (rc = t->js_u_val.put(uval)) || (rc = t->js_u_dinv.put(udi)))
        return rc;
    for (Dev<double> *w : {&t->w0, &t->w1, &t->w2})
        if (w->alloc((size_t)(n ? n : 1))) {
            (void)hipGetLastError();
            set_error("schwz_trs_create_sweeps: out of device memory");
            return SCHWZ_ERR_HIP;
        }
    *out = own.release();
    return SCHWZ_OK;
}

int schwz_trs_sweeps(const schwz_trs *t) { return t ? t->sweeps : 0; }

}  // extern "C"
