// The uneven cuts of the z-sweep walks' segment tables (walk_segment_table, csrc/coding_plan.cpp) on geometry alone:
// no matrix, no GPU, no HIP runtime.  For every case and the trims 0, the library's defaults and 300 per mille it
// checks that every (band, position) is covered exactly once, that the table keeps its size and the bands their
// entries (hence their XCDs), that trim 0 is the equal-pieces formula entry for entry, that no late piece is longer
// than an early piece of its run, that no piece falls below the planner's floor unless the equal piece already did,
// and that runs below the threshold keep their equal pieces.  Prints one line per case and trim.
// Built with -fsanitize=address,undefined (make walk_trim_driver); links coding_plan.cpp and host_setup.cpp only.
//   walk_trim_driver [case [trim]] | --list | --env
#include <algorithm>
#include <cstring>
#include <map>
#include <string>

#include "coding_plan.hpp"

using namespace schwz;

namespace {

[[noreturn]] void die(const std::string &msg)
{
    std::fprintf(stderr, "walk_trim_driver: %s\n", msg.c_str());
    std::exit(1);
}
#define CHECK(cond, what) \
    do {                  \
        if (!(cond)) die(std::string(name) + ", trim " + std::to_string(trim) + ": " + what + " (" #cond ")"); \
    } while (0)

// which of the three tables of a plan: its trim's default and the planner's floor for its segment length
enum Table { kUpdate, kDirection, kFirst };

struct Case {
    const char *name;
    std::vector<WalkRun> runs;
    int64_t PL;
    int T, cus, wg_per_cu;
    Table table;
    int asked;  // a segment length as SCHWZ_SWEEP_L would ask for it (0: the planner's own)
};

int table_floor(Table t) { return t == kFirst ? 6 : 8; }
int table_step(Table t) { return t == kFirst ? 2 : 4; }

// the planner's segment length without a request: about wg_per_cu segments per CU, at least the floor
int planner_length(const Case &c)
{
    if (c.asked) return c.asked;
    const int64_t bands = (c.PL + c.T - 1) / c.T;
    int64_t steps = 0;
    for (const WalkRun &r : c.runs) steps += (int64_t)(r.p1 - r.p0) * bands;
    const int64_t wgs = (int64_t)c.wg_per_cu * c.cus;
    return (int)std::max<int64_t>(table_floor(c.table), (steps + wgs - 1) / wgs);
}

// The table before there was a trim, written out again here: equal pieces of ceil(R / nseg) positions, the last one
// the remainder; sorted by first position, then band; XCD x takes the bands [x * bands / 8, (x + 1) * bands / 8)
// (fewer than 16 bands: the shortest list), entry [q * 8 + x] the q-th segment of XCD x.
std::vector<int4> equal_pieces_table(const Case &c, int L)
{
    const int bands = (int)((c.PL + c.T - 1) / c.T);
    struct Seg { int band, p0, p1; };
    std::vector<Seg> segs;
    for (const WalkRun &r : c.runs) {
        const int nseg = (r.p1 - r.p0 + L - 1) / L, len = (r.p1 - r.p0 + nseg - 1) / nseg;
        for (int b = 0; b < bands; ++b)
            for (int p = r.p0; p < r.p1; p += len) segs.push_back({b, p, std::min(p + len, r.p1)});
    }
    std::stable_sort(segs.begin(), segs.end(), [](const Seg &x, const Seg &y) { return x.p0 != y.p0 ? x.p0 < y.p0 : x.band < y.band; });
    std::vector<std::vector<int4>> per_xcd(kXcds);
    for (const Seg &s : segs) {
        int4 v;
        v.x = s.band;
        v.y = s.p0;
        v.z = s.p1;
        v.w = (int)std::min<int64_t>(c.T, c.PL - (int64_t)s.band * c.T);
        size_t x = 0;
        if (bands >= 2 * kXcds) {
            x = (size_t)((int64_t)s.band * kXcds / bands);
        } else {
            for (size_t k = 1; k < (size_t)kXcds; ++k)
                if (per_xcd[k].size() < per_xcd[x].size()) x = k;
        }
        per_xcd[x].push_back(v);
    }
    size_t depth = 0;
    for (const auto &l : per_xcd) depth = std::max(depth, l.size());
    std::vector<int4> out(depth * kXcds);
    for (size_t q = 0; q < depth; ++q)
        for (int x = 0; x < kXcds; ++x) {
            int4 v;
            v.x = v.y = v.z = v.w = 0;
            if (q < per_xcd[(size_t)x].size()) v = per_xcd[(size_t)x][q];
            out[q * kXcds + x] = v;
        }
    return out;
}

bool same(const int4 &a, const int4 &b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// the cuts of run r in a table: first positions of its pieces (those of band 0; every band must repeat them)
std::vector<int> cuts_of(const std::vector<int4> &tab, const WalkRun &r, int band)
{
    std::vector<int> c;
    for (const int4 &v : tab)
        if (v.z > v.y && v.x == band && v.y >= r.p0 && v.y < r.p1) c.push_back(v.y);
    std::sort(c.begin(), c.end());
    return c;
}

void check_case(const Case &c, int trim)
{
    const char *name = c.name;
    const int L = planner_length(c), floor = table_floor(c.table), bands = (int)((c.PL + c.T - 1) / c.T);
    const std::vector<int4> base = equal_pieces_table(c, L);
    const std::vector<int4> zero = walk_segment_table(c.runs, c.PL, c.T, L, c.cus, 0, floor, table_step(c.table), 1 << 30);
    const std::vector<int4> tab = walk_segment_table(c.runs, c.PL, c.T, L, c.cus, trim, floor, table_step(c.table), 1 << 30);
    // trim 0: the equal-pieces formula, entry for entry
    CHECK(zero.size() == base.size(), "trim 0 changes the size of the table");
    for (size_t i = 0; i < base.size(); ++i) CHECK(same(zero[i], base[i]), "trim 0 differs from the equal-pieces formula");
    // the same entries hold the same bands (and their rows): the XCD placement and the slots do not move
    CHECK(tab.size() == base.size(), "the trim changes the size of the table");
    size_t filled = 0;
    for (size_t i = 0; i < base.size(); ++i) {
        CHECK(tab[i].x == base[i].x && tab[i].w == base[i].w, "an entry changed its band");
        CHECK((tab[i].z > tab[i].y) == (base[i].z > base[i].y), "an entry was emptied or filled");
        filled += tab[i].z > tab[i].y;
    }
    // every (band, position) exactly once
    int npos = 0;
    for (const WalkRun &r : c.runs) npos = std::max(npos, r.p1);
    std::vector<int> seen((size_t)bands * npos, 0);
    for (const int4 &v : tab) {
        if (v.z <= v.y) continue;
        CHECK(v.x >= 0 && v.x < bands && v.y >= 0 && v.z <= npos, "segment outside the chain");
        CHECK(v.w == (int)std::min<int64_t>(c.T, c.PL - (int64_t)v.x * c.T), "rows of the band");
        for (int p = v.y; p < v.z; ++p) ++seen[(size_t)v.x * npos + p];
    }
    for (int b = 0; b < bands; ++b)
        for (int p = 0; p < npos; ++p) {
            bool in_run = false;
            for (const WalkRun &r : c.runs) in_run |= p >= r.p0 && p < r.p1;
            CHECK(seen[(size_t)b * npos + p] == (in_run ? 1 : 0), "a position is covered twice or not at all");
        }
    // per run: the same cuts in every band; pieces inside the run; late pieces (those that got shorter than the
    // equal piece... or stayed) never longer than an early one; the floor; the threshold
    int moved = 0;
    std::string lens;
    for (const WalkRun &r : c.runs) {
        const std::vector<int> cut = cuts_of(tab, r, 0), cut0 = cuts_of(base, r, 0);
        CHECK(cut.size() == cut0.size() && !cut.empty() && cut[0] == r.p0, "number of pieces of a run");
        for (int b = 1; b < bands; ++b) CHECK(cuts_of(tab, r, b) == cut, "bands of a run are cut differently");
        const int R = r.p1 - r.p0, nseg = (int)cut.size(), equal = (R + nseg - 1) / nseg;
        std::vector<int> len((size_t)nseg), len0((size_t)nseg);
        for (int k = 0; k < nseg; ++k) {
            len[(size_t)k] = (k + 1 < nseg ? cut[(size_t)k + 1] : r.p1) - cut[(size_t)k];
            len0[(size_t)k] = (k + 1 < nseg ? cut0[(size_t)k + 1] : r.p1) - cut0[(size_t)k];
            lens += (k ? " " : (lens.empty() ? "" : " | ")) + std::to_string(len[(size_t)k]);
        }
        if (equal < kWalkTrimMinLen || trim == 0) {
            CHECK(len == len0, "a run below the threshold (or trim 0) was cut differently");
            continue;
        }
        if (len == len0) continue;  // no late round in this run
        // Late pieces are a suffix of the run (the table is in chain order).  Whatever the split point, no piece behind
        // it may be longer than one before it: the lengths never increase along the run.
        for (int k = 1; k < nseg; ++k) CHECK(len[(size_t)k] <= len[(size_t)k - 1], "a later piece is longer than an earlier one");
        for (int k = 0; k < nseg; ++k) {
            CHECK(len[(size_t)k] >= std::min(floor, len0[(size_t)k]), "a piece below the planner's floor");
            moved = std::max(moved, std::abs(cut[(size_t)k] - cut0[(size_t)k]));
        }
    }
    std::printf("%s trim %d: L %d, %zu entries (%zu filled), %d bands, pieces %s, largest move of a cut %d\n", c.name, trim, L,
                tab.size(), filled, bands, lens.c_str(), moved);
    // a table with at most `cus` segments has no late round
    if ((int)filled <= c.cus)
        for (size_t i = 0; i < base.size(); ++i) CHECK(same(tab[i], base[i]), "a table of at most one round was trimmed");
}

std::vector<Case> cases()
{
    const std::vector<WalkRun> cube = {{0, 256}}, slab = {{0, 64}};
    return {
        // the flagship, 256^3: planes of 65536 rows, one run of 256 positions, 256 CUs
        {"cube_update", cube, 65536, 512, 256, 3, kUpdate, 0},
        {"cube_direction", cube, 65536, 1024, 256, 2, kDirection, 0},
        {"cube_first", cube, 65536, 512, 256, 6, kFirst, 0},
        // the 512 x 512 x 64 slab of the multi-GPU runs: planes of 262144 rows in bands of 1024
        {"slab_update", slab, 262144, 1024, 256, 2, kUpdate, 0},
        {"slab_first", slab, 262144, 1024, 256, 6, kFirst, 0},
        // a middle slab: the interior planes and, chained behind a gap, the appended overlap planes
        {"two_runs", {{0, 130}, {131, 195}}, 65536, 512, 256, 3, kUpdate, 0},
        {"two_runs_short_tail", {{0, 200}, {202, 214}}, 65536, 1024, 256, 2, kDirection, 0},
        // another device
        {"cube_update_cus64", cube, 65536, 512, 64, 3, kUpdate, 0},
        {"cube_first_cus64", cube, 65536, 512, 64, 6, kFirst, 0},
        {"cube_update_cus304", cube, 65536, 512, 304, 3, kUpdate, 0},
        // the threshold: equal pieces of 15 positions are left alone, of 16 are trimmed
        {"below_threshold", {{0, 90}}, 65536, 512, 256, 0, kUpdate, 15},
        {"at_threshold", {{0, 96}}, 65536, 512, 256, 0, kUpdate, 16},
        // a partial last band and an asked length (planes that are not whole chunks)
        {"partial_band_asked_20", {{0, 40}}, 1800, 512, 256, 0, kUpdate, 20},
        // the shapes of tests/test_gpu_walk_trim.py: 40 planes, a length of 20 asked for, tables planned for three CUs
        {"gpu_256x4x40", {{1, 41}}, 1024, 512, 3, 0, kUpdate, 20},
        {"gpu_200x9x40", {{1, 41}}, 1800, 512, 3, 0, kUpdate, 20},
        {"gpu_200x9x40_direction", {{1, 41}}, 1800, 1024, 3, 0, kDirection, 20},
    };
}

}  // namespace

int main(int argc, char **argv)
{
    const std::vector<Case> all = cases();
    if (argc > 1 && !std::strcmp(argv[1], "--list")) {
        for (const Case &c : all) std::printf("%s\n", c.name);
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "--env")) {  // the three trims as SCHWZ_SWEEP_TRIM sets them
        const CodingOptions o = coding_options_from_env();
        std::printf("%d %d %d\n", o.sweep_trim, o.sweep_trim_dir, o.sweep_trim_first);
        return 0;
    }
    const CodingOptions def;
    std::printf("defaults update %d direction %d first %d\n", def.sweep_trim, def.sweep_trim_dir, def.sweep_trim_first);
    int ran = 0;
    for (const Case &c : all) {
        if (argc > 1 && std::strcmp(argv[1], c.name)) continue;
        const int d = c.table == kUpdate ? def.sweep_trim : (c.table == kDirection ? def.sweep_trim_dir : def.sweep_trim_first);
        if (argc > 2) check_case(c, std::atoi(argv[2]));
        else for (int trim : {0, d, 300}) check_case(c, trim);
        ++ran;
    }
    if (!ran) die("no such case");
    return 0;
}
