// Host plan of the aggregation coarse correction (coarse_plan.hpp) and the dense inverse of A0.  No HIP runtime
// call; threads from setup_threads() (SCHWZ_SETUP_THREADS).  Every sum is formed in an order that depends on the
// data alone -- rows ascending, slots ascending -- so the plan is the same bits for any thread count.
#include "coarse_plan.hpp"

#include <cmath>
#include <limits>

namespace schwz {

int plan_coarse(int64_t local_size, int64_t nslots, const schwz_idx *rp, const schwz_idx *col, const double *val,
                const double *rhs, const int32_t *slot_agg, int32_t first_agg, int32_t m, int32_t nc, CoarsePlan *out)
{
    SCHWZ_REQUIRE(out, "plan_coarse: null output");
    SCHWZ_REQUIRE(nc >= 1 && nc <= kCoarseMaxDofs,
                  "plan_coarse: the number of aggregates must be in [1, " + std::to_string(kCoarseMaxDofs) + "]");
    SCHWZ_REQUIRE(first_agg >= 0 && m >= 0 && (int64_t)first_agg + m <= nc,
                  "plan_coarse: the subdomain's aggregate range lies outside [0, nc)");
    SCHWZ_REQUIRE(local_size >= 0 && nslots >= local_size, "plan_coarse: bad sizes");
    SCHWZ_REQUIRE(nslots == 0 || slot_agg, "plan_coarse: null aggregate ids");
    SCHWZ_REQUIRE(local_size == 0 || (rp && col && val && rhs), "plan_coarse: null matrix or right-hand side");
    for (int64_t j = 0; j < nslots; ++j) {
        SCHWZ_REQUIRE(slot_agg[j] >= 0 && slot_agg[j] < nc, "plan_coarse: a slot's aggregate id lies outside [0, nc)");
        SCHWZ_REQUIRE(j >= local_size || (slot_agg[j] >= first_agg && slot_agg[j] - first_agg < m),
                      "plan_coarse: an interior row belongs to an aggregate outside the subdomain's own range");
    }
    for (int64_t i = 0; i < local_size; ++i)
        for (schwz_idx k = rp[i]; k < rp[i + 1]; ++k)
            SCHWZ_REQUIRE(col[k] >= 0 && col[k] < nslots, "plan_coarse: a column of an interior row is no x~ slot");
    CoarsePlan &p = *out;
    p = CoarsePlan();
    p.first_agg = first_agg;
    p.m = m;
    p.nc = nc;
    p.nslots = nslots;
    p.id16.resize((size_t)nslots);
    for (int64_t j = 0; j < nslots; ++j) p.id16[(size_t)j] = (uint16_t)slot_agg[j];
    // the rows of every aggregate, ascending (counting sort)
    std::vector<int64_t> row_ptr((size_t)m + 1, 0);
    for (int64_t i = 0; i < local_size; ++i) ++row_ptr[(size_t)(slot_agg[i] - first_agg) + 1];
    for (int32_t a = 0; a < m; ++a) row_ptr[(size_t)a + 1] += row_ptr[(size_t)a];
    std::vector<schwz_idx> rows_of((size_t)local_size);
    {
        std::vector<int64_t> fill(row_ptr.begin(), row_ptr.end() - 1);
        for (int64_t i = 0; i < local_size; ++i) rows_of[(size_t)fill[(size_t)(slot_agg[i] - first_agg)]++] = (schwz_idx)i;
    }
    p.beta.assign((size_t)m, 0.0);
    p.rows.assign((size_t)m * (size_t)nc, 0.0);
    std::vector<std::vector<int32_t>> ws((size_t)m);
    std::vector<std::vector<double>> wv((size_t)m);
    parallel_blocks(m, 1, [&](int, int, int64_t a0, int64_t a1) {
        std::vector<std::pair<int32_t, double>> ent;
        for (int64_t a = a0; a < a1; ++a) {
            ent.clear();
            double beta = 0.0;
            for (int64_t q = row_ptr[(size_t)a]; q < row_ptr[(size_t)a + 1]; ++q) {
                const int64_t i = rows_of[(size_t)q];
                beta += rhs[i];
                for (schwz_idx k = rp[i]; k < rp[i + 1]; ++k) ent.emplace_back((int32_t)col[k], val[k]);
            }
            p.beta[(size_t)a] = beta;
            // by slot, the rows of a slot staying in ascending order: W_aj is summed row after row
            typedef std::pair<int32_t, double> Entry;
            std::stable_sort(ent.begin(), ent.end(), [](const Entry &x, const Entry &y) { return x.first < y.first; });
            double *row = p.rows.data() + (size_t)a * (size_t)nc;
            for (size_t e = 0; e < ent.size();) {
                const int32_t j = ent[e].first;
                double s = 0.0;
                for (; e < ent.size() && ent[e].first == j; ++e) s += ent[e].second;
                if (s == 0.0) continue;
                ws[(size_t)a].push_back(j);
                wv[(size_t)a].push_back(s);
                row[slot_agg[j]] += s;  // A0[a, agg(j)] += W[a, j], slots ascending
            }
        }
    });
    p.w_ptr.assign((size_t)m + 1, 0);
    p.piece_ptr.assign((size_t)m + 1, 0);
    int64_t total = 0;
    for (int32_t a = 0; a < m; ++a) total += (int64_t)ws[(size_t)a].size();
    SCHWZ_REQUIRE(total < std::numeric_limits<int32_t>::max(), "plan_coarse: W exceeds 2^31-1 entries");
    p.w_slot.reserve((size_t)total);
    p.w_val.reserve((size_t)total);
    for (int32_t a = 0; a < m; ++a) {
        p.w_slot.insert(p.w_slot.end(), ws[(size_t)a].begin(), ws[(size_t)a].end());
        p.w_val.insert(p.w_val.end(), wv[(size_t)a].begin(), wv[(size_t)a].end());
        p.w_ptr[(size_t)a + 1] = (int32_t)p.w_slot.size();
        for (int32_t b = p.w_ptr[(size_t)a]; b < p.w_ptr[(size_t)a + 1]; b += kCoarsePieceCap)
            p.pieces.push_back({a, b, std::min<int32_t>(b + kCoarsePieceCap, p.w_ptr[(size_t)a + 1])});
        p.piece_ptr[(size_t)a + 1] = (int32_t)p.pieces.size();
    }
    return SCHWZ_OK;
}

int group_rows_by_aggregate(int64_t local_size, const uint16_t *id16, int32_t first_agg, int32_t m, AggRows *out)
{
    SCHWZ_REQUIRE(out, "group_rows_by_aggregate: null output");
    SCHWZ_REQUIRE(local_size >= 0 && m >= 0 && (local_size == 0 || id16), "group_rows_by_aggregate: bad arguments");
    SCHWZ_REQUIRE(local_size < (int64_t)std::numeric_limits<int32_t>::max(),
                  "group_rows_by_aggregate: more than 2^31-1 interior rows");
    const int64_t n = local_size;
    out->ptr.assign((size_t)m + 1, 0);
    out->rows.assign((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t a = (int32_t)id16[(size_t)i] - first_agg;
        SCHWZ_REQUIRE(a >= 0 && a < m, "group_rows_by_aggregate: an interior row's aggregate lies outside the subdomain's range");
        ++out->ptr[(size_t)a + 1];
    }
    for (int32_t a = 0; a < m; ++a) out->ptr[(size_t)a + 1] += out->ptr[(size_t)a];
    std::vector<int32_t> fill(out->ptr.begin(), out->ptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) out->rows[(size_t)fill[(size_t)((int32_t)id16[(size_t)i] - first_agg)]++] = (int32_t)i;
    return SCHWZ_OK;
}

int plan_row_pieces(int32_t m, const int32_t *agg_ptr, std::vector<CoarsePiece> *pieces, std::vector<int32_t> *piece_ptr)
{
    SCHWZ_REQUIRE(pieces && piece_ptr && m >= 0 && agg_ptr, "plan_row_pieces: bad arguments");
    SCHWZ_REQUIRE(agg_ptr[0] == 0, "plan_row_pieces: the offsets do not start at 0");
    pieces->clear();
    piece_ptr->assign((size_t)m + 1, 0);
    for (int32_t a = 0; a < m; ++a) {
        SCHWZ_REQUIRE(agg_ptr[a + 1] >= agg_ptr[a], "plan_row_pieces: the offsets do not ascend");
        for (int32_t b = agg_ptr[a]; b < agg_ptr[a + 1]; b += kCoarsePieceCap)
            pieces->push_back({a, b, (int32_t)std::min<int64_t>((int64_t)b + kCoarsePieceCap, agg_ptr[a + 1])});
        (*piece_ptr)[(size_t)a + 1] = (int32_t)pieces->size();
    }
    return SCHWZ_OK;
}

int dense_inverse(int32_t n, const double *a, double *inv)
{
    SCHWZ_REQUIRE(n >= 0 && (n == 0 || (a && inv)), "schwz_dense_inverse: bad arguments");
    if (n == 0) return SCHWZ_OK;
    const size_t N = (size_t)n;
    std::vector<double> lu(a, a + N * N);
    std::vector<int32_t> perm(N);
    double amax = 0.0;
    for (size_t k = 0; k < N * N; ++k) {
        if (!std::isfinite(lu[k])) amax = std::numeric_limits<double>::infinity();
        amax = std::max(amax, std::fabs(lu[k]));
    }
    for (int32_t i = 0; i < n; ++i) perm[(size_t)i] = i;
    const double tiny = std::isfinite(amax) ? amax * (double)n * std::numeric_limits<double>::epsilon() : amax;
    const char *singular =
        "schwz_dense_inverse: zero, negligible or non-finite pivot -- the coarse matrix A0 = Z^T A Z is singular: the "
        "global matrix is singular (a pure Neumann problem) or an aggregate has no rows";
    for (int32_t k = 0; k < n; ++k) {
        int32_t piv = k;
        double best = std::fabs(lu[(size_t)k * N + k]);
        for (int32_t i = k + 1; i < n; ++i) {
            const double v = std::fabs(lu[(size_t)i * N + k]);
            if (v > best) best = v, piv = i;
        }
        if (!(best > tiny) || !std::isfinite(best)) {
            set_error(singular);
            return SCHWZ_ERR_INVALID;
        }
        if (piv != k) {
            std::swap_ranges(lu.begin() + (size_t)k * N, lu.begin() + (size_t)(k + 1) * N, lu.begin() + (size_t)piv * N);
            std::swap(perm[(size_t)k], perm[(size_t)piv]);
        }
        const double *rk = lu.data() + (size_t)k * N;
        const double d = 1.0 / rk[k];
        // rows below k are independent of each other: any split over threads gives the same bits
        parallel_blocks(n - k - 1, 128, [&](int, int, int64_t i0, int64_t i1) {
            for (int64_t i = k + 1 + i0; i < k + 1 + i1; ++i) {
                double *ri = lu.data() + (size_t)i * N;
                const double l = ri[k] * d;
                ri[k] = l;
                if (l != 0.0)
                    for (int32_t j = k + 1; j < n; ++j) ri[j] -= l * rk[j];
            }
        });
    }
    // X = U^-1 L^-1 P, column block after column block (the columns are independent)
    std::fill(inv, inv + N * N, 0.0);
    for (int32_t i = 0; i < n; ++i) inv[(size_t)i * N + (size_t)perm[(size_t)i]] = 1.0;
    parallel_blocks(n, 32, [&](int, int, int64_t j0, int64_t j1) {
        for (int32_t i = 1; i < n; ++i) {
            double *xi = inv + (size_t)i * N;
            for (int32_t k = 0; k < i; ++k) {
                const double l = lu[(size_t)i * N + k];
                if (l == 0.0) continue;
                const double *xk = inv + (size_t)k * N;
                for (int64_t j = j0; j < j1; ++j) xi[j] -= l * xk[j];
            }
        }
        for (int32_t i = n - 1; i >= 0; --i) {
            double *xi = inv + (size_t)i * N;
            for (int32_t k = i + 1; k < n; ++k) {
                const double u = lu[(size_t)i * N + k];
                if (u == 0.0) continue;
                const double *xk = inv + (size_t)k * N;
                for (int64_t j = j0; j < j1; ++j) xi[j] -= u * xk[j];
            }
            const double d = lu[(size_t)i * N + i];
            for (int64_t j = j0; j < j1; ++j) xi[j] /= d;
        }
    });
    for (size_t k = 0; k < N * N; ++k)
        if (!std::isfinite(inv[k])) {
            set_error(singular);
            return SCHWZ_ERR_INVALID;
        }
    return SCHWZ_OK;
}

}  // namespace schwz

extern "C" int schwz_dense_inverse(int32_t n, const double *h_a, double *h_inv) { return schwz::dense_inverse(n, h_a, h_inv); }
