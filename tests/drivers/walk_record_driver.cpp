// What the z-sweep walk kernels read at entry (csrc/coding_plan.cpp, plan_walk): the per-slot records of the three
// segment tables and the slot tables in the form the kernels stage.  Plans the codings of a few Laplacians on the CPU
// (no GPU, no HIP runtime) and checks, for every slot of all three tables, that the record repeats the int4 entry and
// carries chain_plane[z0 - 1 + k], k = 0 .. 4, as it is -- -1 at the ends of a chain and past the end of the table's
// last run -- and that an empty slot has z0 == z1; for every pattern and slot of both ready tables,
// that the value is canon_val / canon_sym_val bit for bit where the mask has the bit and has all 64 bits clear where it
// has not.  One line per case says what was seen; tests/test_walk_record.py reads them.
// Built with -fsanitize=address,undefined (make walk_record_driver); links coding_plan.cpp and host_setup.cpp only.
//   walk_record_driver [case] | --list
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
    std::fprintf(stderr, "walk_record_driver: %s\n", msg.c_str());
    std::exit(1);
}
#define CHECK(cond, what) \
    do {                  \
        if (!(cond)) die(std::string("invariant broken: ") + what + " (" #cond ")"); \
    } while (0)

// the local matrix of subdomain `me` of P row blocks of a 3-D Laplacian (P = 1: the whole grid)
Csr laplacian(int64_t nx, int64_t ny, int64_t nz, int P, int me, int overlap)
{
    schwz_problem *prob = nullptr;
    if (schwz_problem_laplacian(3, nx, ny, nz, &prob)) die(schwz_last_error());
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

struct Case {
    const char *name;
    Csr (*matrix)();
    int T, L, Ldir, cus, trim;  // SCHWZ_SWEEP_T / L / LDIR (0: the planner's), CUs planned for, trim of all three tables
    bool gen, ahead, uneven;
};

const Case kCases[] = {
    // whole-chunk planes, short segments, segments that begin at a chain end
    {"cube_256x4x12", [] { return laplacian(256, 4, 12, 1, 0, 2); }, 512, 4, 0, 256, 0, false, false, false},
    // planes that are not whole chunks: a partial last band
    {"cube_200x9x11", [] { return laplacian(200, 9, 11, 1, 0, 2); }, 0, 0, 0, 256, 0, true, false, false},
    // the middle slab of three: the appended overlap planes are the two ends of the chain (12, 0 .. 11, 13), its last
    // segment has two positions: -1 behind the chain and in the entries appended to chain_plane inside the lookahead
    {"slab_256x4x36_P3_me1", [] { return laplacian(256, 4, 36, 3, 1, 2); }, 512, 4, 0, 256, 0, false, true, false},
    // a table with a late round (three CUs) and trimmed, unequal pieces: 40 positions cut 22 + 18
    {"cube_256x4x40_trimmed", [] { return laplacian(256, 4, 40, 1, 0, 2); }, 512, 20, 20, 3, 200, false, false, true},
};

struct Seen {
    // -1 among the plane fields: before the segment's first position (it begins at a chain end), ahead of it (k >= 2),
    // ahead with a plane behind it (between two chains), ahead in the four entries appended behind the last chain
    int slots = 0, empty = 0, minus_first = 0, minus_ahead = 0, minus_between = 0, minus_appended = 0;
    std::vector<int> lengths;  // distinct segment lengths
};

// records of one table against its int4 entries and chain_plane
Seen check_records(const std::vector<int4> &seg, const std::vector<WalkRecord> &rec, const std::vector<int> &chain)
{
    Seen s;
    CHECK(rec.size() == seg.size(), "one record per slot");
    for (size_t i = 0; i < seg.size(); ++i) {
        const WalkRecord &r = rec[i];
        CHECK(r.band == seg[i].x && r.z0 == seg[i].y && r.z1 == seg[i].z && r.rows == seg[i].w, "record repeats the segment entry of slot " + std::to_string(i));
        CHECK(r.pad[0] == 0 && r.pad[1] == 0 && r.pad[2] == 0, "padding is zero");
        ++s.slots;
        if (seg[i].y == seg[i].z) {
            CHECK(r.z0 == r.z1, "empty slot has z0 == z1");
            ++s.empty;
            continue;
        }
        CHECK(r.z0 >= 1 && (size_t)r.z0 + 3 < chain.size(), "five positions around z0 inside chain_plane");
        for (int k = 0; k < 5; ++k)
            CHECK(r.plane[k] == chain[(size_t)(r.z0 - 1 + k)], "plane " + std::to_string(k) + " of slot " + std::to_string(i) + " is chain_plane[z0 - 1 + k]");
        CHECK(r.plane[1] >= 0, "the segment's first position has a plane");
        s.minus_first += r.plane[0] < 0;
        for (int k = 2; k < 5; ++k) {
            if (r.plane[k] >= 0) continue;
            ++s.minus_ahead;
            for (int j = k + 1; j < 5; ++j)
                if (r.plane[j] >= 0) {
                    ++s.minus_between;
                    break;
                }
            if ((size_t)(r.z0 - 1 + k) + 4 >= chain.size()) ++s.minus_appended;
        }
        const int len = r.z1 - r.z0;
        if (std::find(s.lengths.begin(), s.lengths.end(), len) == s.lengths.end()) s.lengths.push_back(len);
    }
    std::sort(s.lengths.begin(), s.lengths.end());
    return s;
}

// a ready table against values and masks: `slots` per pattern
int check_ready(const std::vector<double> &ready, const std::vector<double> &val, const std::vector<int> &mask, int slots)
{
    CHECK(ready.size() == val.size() && val.size() == mask.size() * (size_t)slots * 2, "ready table has the size of the values");
    int absent = 0;
    for (size_t q = 0; q < mask.size(); ++q)
        for (int k = 0; k < slots; ++k)
            for (int b = 0; b < 2; ++b) {
                const size_t e = (q * slots + k) * 2 + b;
                uint64_t got, want;
                std::memcpy(&got, &ready[e], 8);
                std::memcpy(&want, &val[e], 8);
                if ((mask[q] >> (16 * b + k)) & 1) {
                    CHECK(got == want, "present slot holds the value bit for bit");
                } else {
                    CHECK(got == 0, "absent slot holds +0.0, all 64 bits clear");
                    ++absent;
                }
            }
    return absent;
}

void print_seen(const char *table, const Seen &s)
{
    std::printf(" %s slots %d empty %d minus_first %d minus_ahead %d minus_between %d minus_appended %d lengths", table, s.slots,
                s.empty, s.minus_first, s.minus_ahead, s.minus_between, s.minus_appended);
    for (int l : s.lengths) std::printf(" %d", l);
    std::printf(";");
}

void run_case(const Case &c)
{
    const Csr A = c.matrix();
    const int64_t nrows = A.nrows();
    // row tiles and the run length of the XCD deal as schwz_csr_create hands them to the plans (tests/drivers/coding_plan_driver.cpp)
    std::vector<schwz_idx> tiles{0};
    for (int64_t r = 0; r < nrows;) {
        int64_t e = r;
        while (e < nrows && e - r < kTileRows && A.rp[(size_t)e + 1] - A.rp[(size_t)r] <= kTileNnz - 2) ++e;
        if (e == r) e = r + 1;
        tiles.push_back((schwz_idx)e);
        r = e;
    }
    const int ntl = (int)tiles.size() - 1;
    CodingOptions opt;
    opt.pattern = opt.pair = opt.sweep = 2;
    if (c.T) opt.sweep_T = c.T;
    if (c.L) opt.sweep_L = c.L;
    if (c.Ldir) opt.sweep_Ldir = c.Ldir;
    opt.sweep_trim = opt.sweep_trim_dir = opt.sweep_trim_first = c.trim;
    const HostCsr M{nrows, nrows, A.rp.data(), A.col.data(), A.val.data(), tiles};
    const PatternPlan pat = plan_patterns(opt, M);
    PairPlan pair;
    CHECK(pat.built && plan_pair_tables(opt, M, pair), "the matrix is pair coded");
    plan_pair_records(opt, M, 0, pair);
    const WalkPlan W = plan_walk(opt, pair, nrows, nrows, walk_grid(ntl), c.cus, kDirdotHaloLines);
    CHECK(W.built(), "the matrix walks: " + W.why);
    CHECK((W.gen_mode != 0) == c.gen, "generic planes where expected");
    std::printf("%s:", c.name);
    const Seen su = check_records(W.seg, W.rec, W.chain_plane);
    print_seen("update", su);
    CHECK(W.rec_dir.empty() == W.seg_dir.empty() && W.rec_first.empty() == W.seg_first.empty(), "an empty table has no records (it aliases the table before it)");
    Seen sd = su;
    if (!W.seg_dir.empty()) sd = check_records(W.seg_dir, W.rec_dir, W.chain_plane);
    print_seen("direction", sd);
    Seen sf = sd;
    if (!W.seg_first.empty()) sf = check_records(W.seg_first, W.rec_first, W.chain_plane);
    print_seen("first", sf);
    for (const Seen *s : {&su, (const Seen *)&sd, (const Seen *)&sf}) {
        CHECK(s->minus_first > 0, "segments that begin at a chain's first position");
        CHECK(!c.ahead || s == &su || s->slots > 0, "tables exist");
    }
    CHECK(!c.ahead || (su.minus_ahead > 0 && su.minus_appended > 0), "-1 behind the chain's end inside the lookahead of a short last segment");
    CHECK(!c.uneven || su.lengths.size() >= 2, "the trimmed update table has unequal segments");
    const int absent = check_ready(W.canon_ready, W.canon_val, W.canon_mask, 9);
    CHECK(absent > 0, "some pattern lacks a slot");
    CHECK(!W.canon_sym_val.empty() && !W.canon_sym_ready.empty(), "a Laplacian has upper-triangle twins");
    const int absent_sym = check_ready(W.canon_sym_ready, W.canon_sym_val, W.canon_sym_mask, 5);
    std::printf(" ready npat %d absent %d sym_absent %d\n", W.npat, absent, absent_sym);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "--list")) {
        for (const Case &c : kCases) std::printf("%s\n", c.name);
        return 0;
    }
    bool any = false;
    for (const Case &c : kCases)
        if (argc < 2 || !std::strcmp(argv[1], c.name)) {
            run_case(c);
            any = true;
        }
    if (!any) die("usage: walk_record_driver [case] | --list");
    return 0;
}
