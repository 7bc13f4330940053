// Plans of the matrix codings of an upload (coding_plan.cpp): which rows are coded how, every table the SpMV
// kernels read, and the z-sweep walk's chains and segments -- as plain host data.  Planning reads no environment
// variable and asks no device (coding_options_from_env is the one reader of the upload-time switches; the number
// of CUs and the launch grid are arguments), so it runs, and is tested, without a GPU.  spmv_dict.hip and
// spmv_pair.hip upload a plan's arrays and bind them to CsrView; they decide nothing.
#pragma once

#include <optional>

#include "schwz_internal.hpp"

namespace schwz {

// ---- limits the codings share with the kernels that stage their tables in LDS ----
constexpr int kDictMax = 256;      // per-entry dictionaries: distinct values / offsets per tile
constexpr int kChunk = 8;          // gathers issued back to back per lane
constexpr int kPatMax = 64;        // row patterns per table
constexpr int kPatEntries = 1024;  // entries per table (npat * lmax)
constexpr int kPairPats = 64;      // pair patterns per table
constexpr int kPairEntries = 512;  // staged entries per table (npat * stride)
constexpr int kPairChunk = 8;      // gathers issued back to back per lane
constexpr int kPairRows = 2 * kBlock;  // rows per chunk: one pair per lane

__host__ __device__ inline int pat_stride(int lmax) { return (lmax + kChunk - 1) / kChunk * kChunk; }
__host__ __device__ inline int pair_stride(int lmax, int ch = kPairChunk) { return (lmax + ch - 1) / ch * ch; }

// what the launches raise the walk kernels' dynamic-LDS limit to
constexpr size_t kSweepLdsLimit = 96 << 10;

// dynamic LDS of the update / start walk on bands of T rows: the ring (4 T own + 4 NX halo doubles) and the
// nine-slot tables of every pattern
inline size_t sweep_update_lds(int64_t T, int64_t nx, int npat)
{
    return (size_t)(4 * T + 4 * nx) * sizeof(double) + (size_t)npat * (9 * 16 + 4);
}

// NX-row halo lines of p' in the fused direction walk's LDS window: the halo of a position is requested three
// positions ahead -- in the step in which the neighbouring band fetches the same lines as its own window, so they hit
// L2 (spmv_pair.hip, profiles/r03_dd_ab.txt) -- and each of the three in flight needs a slot.  The planning functions
// never read the constant: spmv_pair.hip hands it to plan_walk.
constexpr int kDirdotHaloLines = 3;

// ... of the fused direction walk: `halo_lines` halo lines in its window, the upper triangle's five slots in its tables
inline size_t sweep_dirdot_lds(int64_t T_dir, int64_t nx, int npat, int halo_lines)
{
    return (size_t)(4 * T_dir + halo_lines * nx) * sizeof(double) + (size_t)npat * (5 * 16 + 4);
}

// The upload-time switches (README.md, "Switches"), read once per schwz_csr_create.
struct CodingOptions {
    int pattern = 1, pair = 1, dict = 1;  // SCHWZ_SPMV_PATTERN / PAIR / DICT: 0 off, 2 whatever the coverage; PAIR=3: per-chunk tables
    bool sym = true;                      // SCHWZ_SPMV_SYM
    int rle = 1;                          // SCHWZ_SPMV_RLE: 0 byte ids only, 8 short records only
    bool canon = true;                    // SCHWZ_SPMV_CANON
    int sweep = 1;                        // SCHWZ_SPMV_SWEEP: 0 off, 2 also below 2^20 rows
    bool sweep_gen = true;                // SCHWZ_SWEEP_GEN
    std::optional<int> sweep_T, sweep_L, sweep_Tdir, sweep_Ldir;  // SCHWZ_SWEEP_T / L / TDIR / LDIR
    int sweep_first_per_cu = 6;           // SCHWZ_SWEEP_FIRSTPERCU
    bool sweep_why = false;               // SCHWZ_SWEEP_WHY
    // SCHWZ_SWEEP_TRIM="u,d,f" (one number: all three; 0: equal pieces): per mille by which the pieces of a run whose
    // workgroups are the last dispatched to their CU are shorter than the others (walk_segment_table), for the table of
    // the update and start walks, of the fused direction walk and of the first-direction walk.
    // Defaults (profiles/r17_walk_trim.txt, MI355X, 256^3): the condition prologue + positions x step equal for late and
    // early workgroups on the timeline of the equal pieces gives 124 (update) and 75 (fused direction); in alternating
    // runs 90 and 120 measured the same on the update table (150 slower) and 60 and 90 the same on the fused direction
    // table (30 less, 120 no more): 90 and 60, together -1.3 % per step on the cube and -1.1 % on the 512 x 512 x 64
    // slab against the parent library, each a gain by the rule of r16_walk_launch_constant.txt.  The first-direction
    // walk ends with a workgroup of its FIRST round, which a trim only lengthens: 260 measured nothing and the table
    // keeps equal pieces.
    int sweep_trim = 90, sweep_trim_dir = 60, sweep_trim_first = 0;
    // SCHWZ_SWEEP_CUS: the number of CUs the walk's tables are planned for instead of the device's (a table of at most
    // that many segments is one dispatch round and is never trimmed: this is how a small matrix gets a late round)
    std::optional<int> sweep_cus;
};
CodingOptions coding_options_from_env();

// the matrix as the upload sees it: host CSR and the row tiles of schwz_csr_create
struct HostCsr {
    int64_t nrows, ncols;
    const schwz_idx *rp, *col;
    const double *val;
    const std::vector<schwz_idx> &tiles;
};

// Row-pattern coding (spmv_pattern_kernel).  fraction: share of the nonzeros in coded tiles, known even
// where the coding is not accepted.
struct PatternPlan {
    bool built = false;
    double fraction = 0.0;
    std::vector<uint8_t> pat_id, tbl_len;
    std::vector<schwz_idx> tile_table, tbl_desc, tbl_delta;
    std::vector<double> tbl_val;
};
PatternPlan plan_patterns(const CodingOptions &opt, const HostCsr &M);

// Per-entry dictionaries (spmv_dict_kernel): only without row patterns, or when forced.
struct DictPlan {
    bool built = false;
    double fraction = 0.0;
    std::vector<uint16_t> code;
    std::vector<schwz_idx> vptr, dptr, ddict;
    std::vector<double> vdict;
};
DictPlan plan_dict(const CodingOptions &opt, const HostCsr &M, bool patterns_built);

struct PairEntryH {
    schwz_idx off;
    int flags;
    uint64_t va, vb;
    bool operator==(const PairEntryH &o) const { return off == o.off && flags == o.flags && va == o.va && vb == o.vb; }
};

struct PairTable {
    int npat = 0, lmax = 0;
    std::vector<uint8_t> len;
    std::vector<PairEntryH> ent;  // [npat][lmax], padded with {0,0,0,0}
    uint64_t hash = 0;
    bool same(const PairTable &o) const { return npat == o.npat && lmax == o.lmax && len == o.len && ent == o.ent; }
};

// Row-pair coding (spmv_pair_kernel).  plan_pair_tables codes the pairs and decides whether the coding is
// accepted (false: only `fraction` means anything); plan_pair_records completes an accepted plan.
struct PairPlan {
    bool built = false;
    double fraction = 0.0;
    int64_t code_bytes = 0;  // what a pass over the coded matrix reads (schwz_csr_matrix_bytes)
    int single = 0, sym_base = 0, shift = 0, rle_runs = 8;
    int canon[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint8_t> pair_id, ptbl_len;
    std::vector<schwz_idx> chunk_ptable, ptbl_desc, ptbl_meta;
    std::vector<double> ptbl_val;
    std::vector<uint16_t> rle;       // empty: byte ids only
    std::vector<PairTable> tables;   // host form of ptbl_*: what the walk plan reads
};
bool plan_pair_tables(const CodingOptions &opt, const HostCsr &M, PairPlan &P);
void plan_pair_records(const CodingOptions &opt, const HostCsr &M, int deal_shift, PairPlan &P);

// The z-sweep walk over a single-table pair coding.  Not built: seg is empty and `why` says why (empty: the
// coding has per-chunk tables and nobody asked).  seg_dir / seg_first empty: that launch shares the table
// before it (T_dir / T_first and nslots_dir / nslots_first then repeat that table's).
struct WalkPlan {
    std::string why;
    int gen_mode = 0, T = 0, nx = 0, gen_blocks = 0, T_dir = 0, T_first = 0, npat = 0;
    int64_t pl = 0;
    std::vector<int4> seg, seg_dir, seg_first;
    std::vector<schwz_idx> gen;
    std::vector<double> canon_val, canon_sym_val;  // canon_sym_*: empty without upper-triangle twins
    std::vector<int> canon_mask, canon_sym_mask, chain_plane, chain_far;
    // What the kernels read at entry.  rec / rec_dir / rec_first: one WalkRecord per slot of seg / seg_dir / seg_first
    // (empty like them) -- the entry itself and chain_plane[z0 - 1 + k], k = 0 .. 4, copied as they are (-1: no plane;
    // positions before the table's first: -1 too), so the first windows wait for one load, not for two in a row.
    // canon_ready / canon_sym_ready: canon_val / canon_sym_val with +0.0 (all 64 bits clear) wherever the mask has no
    // bit, the form the walks stage into LDS when they sum every slot -- a function of the matrix, made once here
    // instead of by every workgroup of every launch.
    std::vector<WalkRecord> rec, rec_dir, rec_first;
    std::vector<double> canon_ready, canon_sym_ready;
    bool built() const { return !seg.empty(); }
    int nslots() const { return (int)seg.size(); }
    int nslots_dir() const { return seg_dir.empty() ? nslots() : (int)seg_dir.size(); }
    int nslots_first() const { return seg_first.empty() ? nslots_dir() : (int)seg_first.size(); }
};
// The segment table of one walk launch, from geometry alone.  runs: chain positions [p0, p1) of consecutive walkable
// planes of PL rows, cut into bands of T rows; L: the segment length aimed at, raised by `step` until segments + kXcds
// fit `room` slots.  A run of R positions becomes nseg = ceil(R / L) pieces per band, and nseg does not depend on the
// trim: only where the cuts fall does.
//   trim = 0: equal pieces of ceil(R / nseg) positions, the last one the remainder.
//   trim > 0 (per mille, at most kWalkTrimMax): the workgroups dispatched LAST to their CU run every step slower than the
//     others (profiles/r16_walk_timeline.txt), so their pieces are made shorter, len_late ~ (1 - trim / 1000) len_early,
//     and the other pieces of the run share the rest evenly.  Block b reads entry b and the hardware deals the blocks
//     round robin over the XCDs, so those workgroups hold the last `cus` filled entries; in table order (first
//     position, then band) that is a whole number of pieces or nearly so: a piece is late when more than half of its
//     segments are among them.  Untouched: a table of at most `cus` segments (one round), a run whose equal pieces have
//     fewer than kWalkTrimMinLen positions (one position is more than 6 % there), a run without late or without early
//     pieces.  No late piece goes below `floor` positions (the planner's floor of the table) unless the equal piece did.
// Entries {band, p0, p1, rows of the band}, dealt to the XCDs: entry [q * kXcds + x] is the q-th segment of XCD x
// ({0, 0, 0, 0}: none).  Every band of a run has the same cuts, and an entry holds the same band whatever the trim.
struct WalkRun { int p0, p1; };
constexpr int kWalkTrimMinLen = 16;
constexpr int kWalkTrimMax = 500;
std::vector<int4> walk_segment_table(const std::vector<WalkRun> &runs, int64_t PL, int T, int L, int cus, int trim,
                                     int floor, int step, int room);

// grid: workgroups of an SpMV launch on this matrix (their partial-sum slots bound segments + companion workgroups)
inline int walk_grid(int64_t ntiles) { return (int)((std::min<int64_t>(ntiles, kMaxGrid) + kXcds - 1) / kXcds) * kXcds; }
WalkPlan plan_walk(const CodingOptions &opt, const PairPlan &P, int64_t nrows, int64_t ncols, int grid, int cus,
                   int dirdot_halo_lines);

// Fused dual residual: the chunks whose rows or columns reach `split`, and for a walk over whole-chunk planes of
// walk_pl rows (0: none) the flagged chain positions, their planes' chunks and the workgroups of that launch.
struct DualPlan {
    std::vector<uint8_t> chunk_dual;
    std::vector<int> chain_dual;  // empty (with dual_chunks): no plane is flagged
    std::vector<schwz_idx> dual_chunks;
    int dual_blocks = 0;
};
DualPlan plan_dual_split(int64_t nrows, const schwz_idx *rp, const schwz_idx *col, int64_t split,
                         const std::vector<int> &chain_plane, int64_t walk_pl);

}  // namespace schwz
