// Plan of the aggregation coarse correction of one subdomain (coarse_plan.cpp), as plain host data: what
// coarse.hip uploads and its kernels read.  Planning makes no HIP runtime call and reads no environment variable
// but SCHWZ_SETUP_THREADS (through setup_threads()), so it runs, and is tested, without a GPU; its result does not
// depend on the thread count.
//
// Z is the 0/1 matrix of a partition of the global rows into nc aggregates, each inside the interior of one
// subdomain; this subdomain owns the aggregates [first_agg, first_agg + m).  With x~ holding current global values
// in all its slots, the coarse residual of an own aggregate a is
//     (Z^T (b - A x))_a = beta_a - sum_j W_aj x~_j,   beta_a = sum_{i in a} b_i,   W_aj = sum_{i in a} A_ij
// over the interior rows i of the local matrix (their columns are x~ slots).  Exact zeros of W are dropped: on a
// stencil only slots next to an aggregate's faces or to the domain boundary remain.
#pragma once

#include "schwz_internal.hpp"

namespace schwz {

constexpr int kCoarseMaxDofs = 4096;   // nc: aggregate ids fit 16 bits, c fits LDS, the explicit inverse stays <= 128 MB
constexpr int kCoarsePieceCap = 2048;  // W entries, or rows of an aggregate, one workgroup reduces

struct CoarsePiece {
    int32_t agg, begin, end;  // local aggregate and its W entries [begin, end), end - begin <= kCoarsePieceCap
};

struct CoarsePlan {
    int32_t first_agg = 0, m = 0, nc = 0;
    int64_t nslots = 0;
    std::vector<double> beta;           // m
    std::vector<int32_t> w_ptr;         // m + 1: entries of aggregate a are [w_ptr[a], w_ptr[a + 1]), slots ascending
    std::vector<int32_t> w_slot;
    std::vector<double> w_val;
    std::vector<CoarsePiece> pieces;    // aggregate after aggregate, entries ascending
    std::vector<int32_t> piece_ptr;     // m + 1: pieces of aggregate a are [piece_ptr[a], piece_ptr[a + 1])
    std::vector<uint16_t> id16;         // nslots: global aggregate of every x~ slot
    std::vector<double> rows;           // m x nc, row-major: the subdomain's rows of A0 = Z^T A Z
};

// rp / col / val: the local matrix (rows [0, local_size) are read), rhs: b on those rows, slot_agg: the global
// aggregate id of every x~ slot (nslots of them).  SCHWZ_ERR_INVALID (message set) for nc outside [1, kCoarseMaxDofs],
// an id range outside [0, nc), a slot id outside [0, nc) or an interior slot outside the subdomain's own range.
int plan_coarse(int64_t local_size, int64_t nslots, const schwz_idx *rp, const schwz_idx *col, const double *val,
                const double *rhs, const int32_t *slot_agg, int32_t first_agg, int32_t m, int32_t nc, CoarsePlan *out);

// The interior rows grouped by aggregate, and their cut into pieces: what schwz_ras_rhs_aggregate (ptr, rows) and the
// streaming restriction schwz_ras_aggregate_sums (all four) read.
struct AggRows {
    std::vector<int32_t> ptr;           // m + 1: rows of aggregate a are rows[ptr[a], ptr[a + 1]), ascending
    std::vector<int32_t> rows;          // local_size
    std::vector<CoarsePiece> pieces;    // aggregate after aggregate: entries [begin, end) of `rows`
    std::vector<int32_t> piece_ptr;     // m + 1: pieces of aggregate a are [piece_ptr[a], piece_ptr[a + 1])
};

// id16: the global aggregate of the local_size interior rows (the head of CoarsePlan::id16).  Counting sort: the rows
// of an aggregate stay ascending, as in plan_coarse.  SCHWZ_ERR_INVALID (message set) for 2^31-1 rows or more and for
// a row whose aggregate lies outside [first_agg, first_agg + m).  Fills ptr and rows.
int group_rows_by_aggregate(int64_t local_size, const uint16_t *id16, int32_t first_agg, int32_t m, AggRows *out);

// pieces and piece_ptr from agg_ptr (m + 1 ascending offsets) alone: every aggregate's rows cut front to back into
// pieces of at most kCoarsePieceCap, an aggregate without rows gets no piece.  SCHWZ_ERR_INVALID (message set) for
// offsets that do not ascend from 0.
int plan_row_pieces(int32_t m, const int32_t *agg_ptr, std::vector<CoarsePiece> *pieces, std::vector<int32_t> *piece_ptr);

// inv = a^-1 (n x n, row-major) by LU with partial pivoting and n pairs of triangular solves.  SCHWZ_ERR_INVALID
// (message set) for a zero, negligible or non-finite pivot.
int dense_inverse(int32_t n, const double *a, double *inv);

}  // namespace schwz
