// Plans the matrix codings of one named case on the CPU (csrc/coding_plan.cpp, no GPU, no HIP runtime) and prints
// one line per array an upload would send (name, element count, FNV-1a-64 of its bytes) and one per scalar it would
// write into CsrView / schwz_csr.  tests/test_coding_plan.py compares the lines with those recorded from the
// commit before the plans existed (tests/golden/coding_plan_parent.json).  On every case it also checks, without
// any record, that the pair coding is lossless and that the walk's segment tables cover every row exactly once.
// Built with -fsanitize=address,undefined (make coding_plan_driver); links coding_plan.cpp and host_setup.cpp only.
//   coding_plan_driver <case> | --list
#include <cinttypes>
#include <cstring>
#include <string>

#include "coding_plan.hpp"

using namespace schwz;

namespace {

struct Csr {
    std::vector<schwz_idx> rp, col;
    std::vector<double> val;
    int64_t nrows() const { return (int64_t)rp.size() - 1; }
};

[[noreturn]] void die(const std::string &msg)
{
    std::fprintf(stderr, "coding_plan_driver: %s\n", msg.c_str());
    std::exit(1);
}
#define CHECK(cond, what) \
    do {                  \
        if (!(cond)) die(std::string("invariant broken: ") + what + " (" #cond ")"); \
    } while (0)

// the local matrix of subdomain `me` of P row blocks of a Laplacian, through the entry points of the Python wrappers
// (P = 1: the whole grid; the overlap then adds nothing)
Csr laplacian(int dim, int64_t nx, int64_t ny, int64_t nz, int P, int me, int overlap)
{
    schwz_problem *prob = nullptr;
    if (schwz_problem_laplacian(dim, nx, ny, nz, &prob)) die(schwz_last_error());
    std::vector<int64_t> first((size_t)P + 1);
    if (schwz_partition_regular(schwz_problem_size(prob), P, first.data())) die(schwz_last_error());
    schwz_subdomain *sd = nullptr;
    if (schwz_subdomain_setup(prob, P, me, overlap, first.data(), &sd)) die(schwz_last_error());
    int64_t s[10];
    schwz_subdomain_sizes(sd, s);
    Csr A;
    A.rp.resize((size_t)s[1] + 1);
    A.col.resize((size_t)s[4]);
    A.val.resize((size_t)s[4]);
    if (schwz_subdomain_local_matrix(sd, A.rp.data(), A.col.data(), A.val.data())) die(schwz_last_error());
    delete sd;  // (never on a device here)
    schwz_problem_destroy(prob);
    return A;
}

// 5-point stencil on an n x n grid in natural order: diag(row), west, east, south (-n), north (+n)
template <typename D>
Csr grid5(int n, D diag, double west, double east, double south, double north)
{
    Csr A;
    A.rp.push_back(0);
    for (int r = 0; r < n * n; ++r) {
        const int i = r % n, j = r / n;
        auto put = [&](int c, double v) {
            A.col.push_back(c);
            A.val.push_back(v);
        };
        if (j > 0) put(r - n, south);
        if (i > 0) put(r - 1, west);
        put(r, diag(r));
        if (i < n - 1) put(r + 1, east);
        if (j < n - 1) put(r + n, north);
        A.rp.push_back((schwz_idx)A.col.size());
    }
    return A;
}

struct Case {
    const char *name;
    Csr (*matrix)();
    const char *env;  // "NAME=value ..." on top of SCHWZ_SPMV_PATTERN=2 SCHWZ_SPMV_PAIR=2 SCHWZ_SPMV_SWEEP=2 ("-": no switch at all)
    int cus;
};

const Case kCases[] = {
    {"cube_256x4x12_T512_L4", [] { return laplacian(3, 256, 4, 12, 1, 0, 2); }, "SCHWZ_SWEEP_T=512 SCHWZ_SWEEP_L=4", 256},
    {"cube_256x4x10_T1024", [] { return laplacian(3, 256, 4, 10, 1, 0, 2); }, "SCHWZ_SWEEP_T=1024", 256},
    {"cube_512x4x8_T1024", [] { return laplacian(3, 512, 4, 8, 1, 0, 2); }, "SCHWZ_SWEEP_T=1024", 256},
    // x lines of 1024 entries: the direction launch takes bands of 2048 rows
    {"cube_1024x4x10_T1024", [] { return laplacian(3, 1024, 4, 10, 1, 0, 2); }, "SCHWZ_SWEEP_T=1024", 256},
    // slabs: appended overlap planes, chains that are not in plane order
    {"slab_256x4x30_P3_me0", [] { return laplacian(3, 256, 4, 30, 3, 0, 2); }, "", 256},
    {"slab_256x4x30_P3_me1", [] { return laplacian(3, 256, 4, 30, 3, 1, 2); }, "", 256},
    {"slab_256x4x30_P3_me2", [] { return laplacian(3, 256, 4, 30, 3, 2, 2); }, "", 256},
    {"slab_256x4x36_P3_me1_overlap4", [] { return laplacian(3, 256, 4, 36, 3, 1, 4); }, "", 256},
    // planes that are not whole chunks: byte ids, partial last band
    {"cube_200x9x12", [] { return laplacian(3, 200, 9, 12, 1, 0, 2); }, "", 256},
    // two-dimensional grids: the x line plays the plane
    {"grid_512", [] { return laplacian(2, 512, 512, 1, 1, 0, 2); }, "", 256},
    {"grid_640", [] { return laplacian(2, 640, 640, 1, 1, 0, 2); }, "", 256},
    {"grid_1000_P2_me1", [] { return laplacian(2, 1000, 1000, 1, 2, 1, 2); }, "", 256},
    // three lines per plane: no canonical layout, no walk
    {"cube_256x3x12", [] { return laplacian(3, 256, 3, 12, 1, 0, 2); }, "", 256},
    // non-symmetric: the 64 x 64 convection-diffusion matrix of tests/conftest.py (cx = 6, cy = -3), no twins
    {"convdiff_64", [] { return grid5(64, [](int) { return 8.5; }, -4.0, -1.0, -1.0, -2.5); }, "", 256},
    // no single table for the whole matrix: per-chunk tables, and the same when asked for them
    {"diag_steps_96", [] { return grid5(96, [](int r) { return 4.0 + r / 512; }, -1.0, -1.0, -1.0, -1.0); }, "", 256},
    {"diag_steps256_96", [] { return grid5(96, [](int r) { return 4.0 + r / 256; }, -1.0, -1.0, -1.0, -1.0); }, "", 256},  // (more than 64 pairs in all)
    {"diag_steps_96_pair3", [] { return grid5(96, [](int r) { return 4.0 + r / 512; }, -1.0, -1.0, -1.0, -1.0); }, "SCHWZ_SPMV_PAIR=3", 256},
    // the thresholds and defaults of the flagship workload's size class
    {"default_128x128x64", [] { return laplacian(3, 128, 128, 64, 1, 0, 2); }, "-", 256},
    {"default_128x128x64_cus64", [] { return laplacian(3, 128, 128, 64, 1, 0, 2); }, "-", 64},  // no record: sanitizers only
};

uint64_t fnv1a(const void *p, size_t bytes)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
    return h;
}
template <typename T>
void array(const char *name, const std::vector<T> &v)
{
    std::printf("array %s %zu %016" PRIx64 "\n", name, v.size(), fnv1a(v.data(), v.size() * sizeof(T)));
}
void scalar(const char *name, int64_t v) { std::printf("scalar %s %" PRId64 "\n", name, v); }
void scalar(const char *name, double v) { std::printf("scalar %s %.17g\n", name, v); }

// row r as the pair coding stores it: pattern `id` of table `t`, half `b` (0: row 2i, 1: row 2i + 1)
void check_pair_row(const Csr &A, const PairPlan &P, int t, int id, int64_t r, int b)
{
    const schwz_idx *d = &P.ptbl_desc[(size_t)t * 5];
    CHECK(id < d[2], "pattern id inside its table");
    int64_t j = A.rp[(size_t)r];
    for (int k = 0; k < (int)P.ptbl_len[(size_t)d[1] + id]; ++k) {
        const size_t e = (size_t)d[0] + (size_t)id * d[3] + k;
        if (!(P.ptbl_meta[2 * e + 1] >> b & 1)) continue;
        CHECK(j < A.rp[(size_t)r + 1] && A.col[(size_t)j] == r + P.ptbl_meta[2 * e] &&
                  std::memcmp(&A.val[(size_t)j], &P.ptbl_val[2 * e + b], 8) == 0,
              "pair tables give back (col, val) of row " + std::to_string(r));
        ++j;
    }
    CHECK(j == A.rp[(size_t)r + 1], "pair tables give back every entry of row " + std::to_string(r));
}

// Decoding pair_id -- or the run-length records where a chunk has them -- through the tables gives back every row
void check_lossless(const Csr &A, const PairPlan &P)
{
    const int64_t nrows = A.nrows(), npairs = (nrows + 1) / 2;
    for (size_t c = 0; c < P.chunk_ptable.size(); ++c) {
        const int t = P.chunk_ptable[c];
        if (t < 0) continue;
        CHECK(!P.single || t == 0, "single-table coding uses table 0");
        const int64_t p0 = (int64_t)c * (kPairRows / 2), p1 = std::min(p0 + kPairRows / 2, npairs);
        const uint16_t *rec = P.rle.empty() || P.rle[c * P.rle_runs] == 0xffffu ? nullptr : &P.rle[c * P.rle_runs];
        for (int64_t p = p0; p < p1; ++p) {
            int id = P.pair_id[(size_t)p];
            if (rec) {
                int k = 0;
                while (k + 1 < P.rle_runs && (rec[k + 1] & 0xff) <= p - p0 && rec[k + 1] != rec[k]) ++k;
                CHECK((rec[k] >> 8) == id, "run-length record and byte id agree");
                id = rec[k] >> 8;
            }
            check_pair_row(A, P, t, id, 2 * p, 0);
            if (2 * p + 1 < nrows) check_pair_row(A, P, t, id, 2 * p + 1, 1);
        }
    }
}

// row r of plane k at chain position p from the nine-slot table of pattern `id`, half b
void check_slot_row(const Csr &A, const WalkPlan &W, int p, int id, int64_t r, int b)
{
    const int k = W.chain_plane[(size_t)p], far = W.chain_far[(size_t)p];
    int64_t off[9] = {0, 0, -W.nx, -1, 0, 1, W.nx, 0, 0};
    for (int s = 0; s < 4; ++s) {  // far slots B0, B1, A0, A1: the same in-plane position of the previous / next chain position's plane
        const int src = far >> (2 * s) & 3, slot = s < 2 ? s : 5 + s;
        off[slot] = src ? ((int64_t)W.chain_plane[(size_t)(src == 1 ? p - 1 : p + 1)] - k) * W.pl : INT64_MIN;
    }
    int64_t j = A.rp[(size_t)r];
    for (int s = 0; s < 9; ++s) {
        if (!(W.canon_mask[(size_t)id] >> (16 * b + s) & 1)) continue;
        CHECK(off[s] != INT64_MIN, "a far slot in use has a window");
        CHECK(j < A.rp[(size_t)r + 1] && A.col[(size_t)j] == r + off[s] &&
                  std::memcmp(&A.val[(size_t)j], &W.canon_val[((size_t)id * 9 + s) * 2 + b], 8) == 0,
              "nine-slot tables give back (col, val) of row " + std::to_string(r));
        ++j;
    }
    CHECK(j == A.rp[(size_t)r + 1], "nine-slot tables give back every entry of row " + std::to_string(r));
}

// every row in exactly one (band, chain position) of one slot of `seg` or in exactly one left-out chunk
void check_cover(const Csr &A, const PairPlan &P, const WalkPlan &W, const std::vector<int4> &seg, int T, int grid, bool slots_too)
{
    const int64_t nrows = A.nrows();
    std::vector<uint8_t> hit((size_t)nrows, 0);
    CHECK(seg.size() % kXcds == 0 && (int64_t)seg.size() + W.gen_blocks <= grid, "slots and companion workgroups within the grid");
    for (const int4 &s : seg) {
        if (s.y == s.z) continue;
        CHECK(s.y < s.z && s.w == std::min<int64_t>(T, W.pl - (int64_t)s.x * T) && s.w > 0, "segment {band, p0, p1, rows} well formed");
        for (int p = s.y; p < s.z; ++p) {
            const int k = W.chain_plane[(size_t)p];
            CHECK(k >= 0, "segment stays inside a chain");
            const int64_t r0 = (int64_t)k * W.pl + (int64_t)s.x * T;
            CHECK(r0 + s.w <= nrows, "band inside the matrix");
            for (int64_t r = r0; r < r0 + s.w; ++r) ++hit[(size_t)r];
            for (int64_t r = r0; slots_too && r < r0 + s.w; r += 2) {
                check_slot_row(A, W, p, P.pair_id[(size_t)(r / 2)], r, 0);
                check_slot_row(A, W, p, P.pair_id[(size_t)(r / 2)], r + 1, 1);
            }
        }
    }
    CHECK(!W.gen_mode || W.gen.empty(), "gen mode leaves no chunk out");
    for (schwz_idx c : W.gen)
        for (int64_t r = (int64_t)c * kPairRows; r < std::min<int64_t>(((int64_t)c + 1) * kPairRows, nrows); ++r) ++hit[(size_t)r];
    for (int64_t r = 0; r < nrows; ++r) CHECK(hit[(size_t)r] == 1, "row " + std::to_string(r) + " covered exactly once");
}

}  // namespace

int main(int argc, char **argv)
{
    const Case *cs = nullptr;
    for (const Case &c : kCases) {
        if (argc == 2 && !std::strcmp(argv[1], "--list")) std::printf("%s\n", c.name);
        if (argc == 2 && !std::strcmp(argv[1], c.name)) cs = &c;
    }
    if (argc == 2 && !std::strcmp(argv[1], "--list")) return 0;
    if (!cs) die("usage: coding_plan_driver <case> | --list");
    for (const char *name : {"SCHWZ_SPMV_PATTERN", "SCHWZ_SPMV_PAIR", "SCHWZ_SPMV_DICT", "SCHWZ_SPMV_SYM", "SCHWZ_SPMV_RLE",
                             "SCHWZ_SPMV_CANON", "SCHWZ_SPMV_SWEEP", "SCHWZ_SWEEP_GEN", "SCHWZ_SWEEP_T", "SCHWZ_SWEEP_L",
                             "SCHWZ_SWEEP_TDIR", "SCHWZ_SWEEP_LDIR", "SCHWZ_SWEEP_FIRSTPERCU", "SCHWZ_SWEEP_WHY"})
        unsetenv(name);
    if (std::strcmp(cs->env, "-")) {
        std::string all = std::string("SCHWZ_SPMV_PATTERN=2 SCHWZ_SPMV_PAIR=2 SCHWZ_SPMV_SWEEP=2 ") + cs->env;
        for (size_t a = 0; a < all.size();) {
            const size_t e = all.find(' ', a) == std::string::npos ? all.size() : all.find(' ', a), q = all.find('=', a);
            if (e > a) setenv(all.substr(a, q - a).c_str(), all.substr(q + 1, e - q - 1).c_str(), 1);
            a = e + 1;
        }
    }
    const Csr A = cs->matrix();
    const int64_t nrows = A.nrows();
    // the row tiles and the run length of the XCD deal, as schwz_csr_create (kernels.hip, which points back here) hands
    // them to the plans; the recorded in_tiles / in_pair_deal_shift lines pin this copy to the commit they were taken from
    std::vector<schwz_idx> tiles{0};
    for (int64_t r = 0; r < nrows;) {
        int64_t e = r;
        while (e < nrows && e - r < kTileRows && A.rp[(size_t)e + 1] - A.rp[(size_t)r] <= kTileNnz - 2) ++e;
        if (e == r) e = r + 1;
        tiles.push_back((schwz_idx)e);
        r = e;
    }
    const int ntl = (int)tiles.size() - 1;
    int deal_shift = 0;
    {
        std::vector<int64_t> bws;
        const int64_t step = nrows > 4096 ? nrows / 4096 : 1;
        for (int64_t i = 0; i < nrows; i += step)
            if (A.rp[(size_t)i + 1] > A.rp[(size_t)i])
                bws.push_back(std::max<int64_t>(i - A.col[(size_t)A.rp[(size_t)i]], A.col[(size_t)A.rp[(size_t)i + 1] - 1] - i));
        int64_t bw = 0;
        if (!bws.empty()) {
            std::nth_element(bws.begin(), bws.begin() + bws.size() / 2, bws.end());
            bw = std::max<int64_t>(0, bws[bws.size() / 2]);
        }
        int64_t B = bw / std::max<int64_t>(1, nrows / std::max(1, ntl)) / kXcds;
        B = std::max<int64_t>(1, std::min<int64_t>(B, (ntl + kXcds - 1) / kXcds));
        while ((int64_t(2) << deal_shift) <= B) ++deal_shift;
    }
    scalar("in_nrows", nrows);
    array("in_rp", A.rp);
    array("in_col", A.col);
    array("in_val", A.val);
    array("in_tiles", tiles);
    scalar("in_pair_deal_shift", (int64_t)deal_shift);

    const CodingOptions opt = coding_options_from_env();
    const HostCsr M{nrows, nrows, A.rp.data(), A.col.data(), A.val.data(), tiles};
    // The driver plans with the halo lines of the fused direction walk (coding_plan.hpp):
    // tests/golden/coding_plan_parent.json was recorded with three.  Whoever changes the number moves the direction
    // tables the record pins, and has to record it anew.
    static_assert(kDirdotHaloLines == 3, "the recorded plans assume the three halo lines of the fused direction walk");
    const int grid = walk_grid(ntl), halo_lines = kDirdotHaloLines;
    // the plans in the order, and under the conditions, of build_spmv_dict / build_spmv_pair
    PatternPlan pat = plan_patterns(opt, M);
    PairPlan pair;
    WalkPlan walk;
    if (pat.built && plan_pair_tables(opt, M, pair)) {
        plan_pair_records(opt, M, deal_shift, pair);
        walk = plan_walk(opt, pair, nrows, nrows, grid, cs->cus, halo_lines);
    }
    const DictPlan dict = plan_dict(opt, M, pat.built);

    if (pair.built) check_lossless(A, pair);
    if (walk.built()) {
        CHECK(sweep_update_lds(walk.T, walk.nx, walk.npat) <= kSweepLdsLimit &&
                  sweep_update_lds(walk.T_first, walk.nx, walk.npat) <= kSweepLdsLimit, "update walk's LDS within 96 KiB");
        CHECK(sweep_dirdot_lds(walk.T_dir, walk.nx, walk.npat, halo_lines) <= kSweepLdsLimit &&
                  sweep_dirdot_lds(walk.T_first, walk.nx, walk.npat, halo_lines) <= kSweepLdsLimit, "direction walk's LDS within 96 KiB");
        check_cover(A, pair, walk, walk.seg, walk.T, grid, true);
        if (!walk.seg_dir.empty()) check_cover(A, pair, walk, walk.seg_dir, walk.T_dir, grid, false);
        if (!walk.seg_first.empty()) check_cover(A, pair, walk, walk.seg_first, walk.T_first, grid, false);
    }
    // the fused dual residual's plan has no record (no upload through schwz.Csr asks for it): run for the sanitizers,
    // and every flagged plane's chunks must be listed
    const DualPlan dual = plan_dual_split(nrows, A.rp.data(), A.col.data(), nrows - nrows / 8, walk.chain_plane,
                                          walk.built() && !walk.gen_mode ? walk.pl : 0);
    CHECK(dual.chunk_dual.size() == (size_t)((nrows + kPairRows - 1) / kPairRows) && dual.chunk_dual.back() == 1, "last chunk reaches the split");
    CHECK(dual.chain_dual.empty() == dual.dual_chunks.empty() && dual.dual_blocks <= 512, "dual chunk list and flags go together");

    // which codings an upload binds, and which launches share the segment table before theirs
    scalar("bound_pat_id", (int64_t)pat.built);
    scalar("bound_code", (int64_t)dict.built);
    scalar("bound_pair_id", (int64_t)pair.built);
    scalar("bound_sweep_seg", (int64_t)walk.built());
    scalar("bound_canon_sym", (int64_t)!walk.canon_sym_val.empty());
    scalar("alias_seg_dir", (int64_t)walk.seg_dir.empty());
    scalar("alias_seg_first", (int64_t)walk.seg_first.empty());
    scalar("pattern_fraction", pat.fraction);
    if (pat.built) {
        array("pat_id", pat.pat_id);
        array("tile_table", pat.tile_table);
        array("tbl_desc", pat.tbl_desc);
        array("tbl_len", pat.tbl_len);
        array("tbl_val", pat.tbl_val);
        array("tbl_delta", pat.tbl_delta);
    }
    scalar("dict_fraction", dict.fraction);
    if (dict.built) {
        array("code", dict.code);
        array("vdict_ptr", dict.vptr);
        array("ddict_ptr", dict.dptr);
        array("vdict", dict.vdict);
        array("ddict", dict.ddict);
    }
    scalar("pair_fraction", pair.fraction);
    if (!pair.built) pair = PairPlan();  // what an upload binds for a coding that was not accepted
    scalar("pair_code_bytes", pair.code_bytes);
    scalar("pair_single", (int64_t)pair.single);
    scalar("pair_sym_base", (int64_t)pair.sym_base);
    scalar("pair_shift", (int64_t)pair.shift);
    scalar("pair_rle_runs", (int64_t)pair.rle_runs);
    for (int k = 0; k < 8; ++k) scalar(("pair_canon" + std::to_string(k)).c_str(), (int64_t)pair.canon[k]);
    if (pair.built) {
        array("pair_id", pair.pair_id);
        array("chunk_ptable", pair.chunk_ptable);
        array("ptbl_desc", pair.ptbl_desc);
        array("ptbl_len", pair.ptbl_len);
        array("ptbl_val", pair.ptbl_val);
        array("ptbl_meta", pair.ptbl_meta);
        if (!pair.rle.empty()) array("pair_rle", pair.rle);
    }
    std::printf("why %s\n", walk.why.c_str());
    scalar("sweep_gen_mode", (int64_t)walk.gen_mode);
    scalar("sweep_T", (int64_t)walk.T);
    scalar("sweep_nx", (int64_t)walk.nx);
    scalar("sweep_pl", walk.pl);
    scalar("sweep_nslots", (int64_t)walk.nslots());
    scalar("sweep_ngen", (int64_t)walk.gen.size());
    scalar("sweep_gen_blocks", (int64_t)walk.gen_blocks);
    scalar("sweep_T_dir", (int64_t)walk.T_dir);
    scalar("sweep_nslots_dir", (int64_t)walk.nslots_dir());
    scalar("sweep_T_first", (int64_t)walk.T_first);
    scalar("sweep_nslots_first", (int64_t)walk.nslots_first());
    scalar("canon_npat", (int64_t)walk.npat);
    if (walk.built()) {
        array("sweep_seg", walk.seg);
        if (!walk.seg_dir.empty()) array("sweep_seg_dir", walk.seg_dir);
        if (!walk.seg_first.empty()) array("sweep_seg_first", walk.seg_first);
        array("sweep_gen", walk.gen);
        array("canon_val", walk.canon_val);
        array("canon_mask", walk.canon_mask);
        if (!walk.canon_sym_val.empty()) {
            array("canon_sym_val", walk.canon_sym_val);
            array("canon_sym_mask", walk.canon_sym_mask);
        }
        array("chain_plane", walk.chain_plane);
        array("chain_far", walk.chain_far);
    }
    return 0;
}
