// The tables of the streaming aggregate restriction (csrc/coarse_plan.cpp: group_rows_by_aggregate, plan_row_pieces)
// on the CPU, as a stand-alone program over coarse_plan.cpp and host_setup.cpp alone, built with the address and
// undefined-behaviour sanitizers (tests/test_row_pieces.py runs it).  A case is a list of aggregate sizes; the rows
// are dealt to the aggregates interleaved (round-robin while an aggregate still wants rows), so no aggregate is one
// contiguous run.  Prints "check <name> pass|fail <figure>" per item and "figure ..." lines.
//   row_pieces_driver --list | <case>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "coarse_plan.hpp"

using namespace schwz;

static int failures = 0;
static void check(const char *name, bool ok, double figure)
{
    std::printf("check %s %s %.0f\n", name, ok ? "pass" : "fail", figure);
    if (!ok) ++failures;
}

// one id per row: round-robin over the aggregates that still want rows
static std::vector<uint16_t> interleave(const std::vector<int32_t> &sizes, int32_t first_agg)
{
    std::vector<int32_t> left(sizes);
    std::vector<uint16_t> id;
    for (bool any = true; any;) {
        any = false;
        for (size_t a = 0; a < left.size(); ++a)
            if (left[a] > 0) {
                --left[a];
                id.push_back((uint16_t)(first_agg + (int32_t)a));
                any = true;
            }
    }
    return id;
}

static void run_case(const std::vector<int32_t> &sizes, int32_t first_agg)
{
    const int32_t m = (int32_t)sizes.size();
    const std::vector<uint16_t> id = interleave(sizes, first_agg);
    const int64_t n = (int64_t)id.size();
    AggRows g;
    if (group_rows_by_aggregate(n, id.data(), first_agg, m, &g) || plan_row_pieces(m, g.ptr.data(), &g.pieces, &g.piece_ptr)) {
        std::printf("check plan fail 0\n%s\n", schwz_last_error());
        ++failures;
        return;
    }
    // the grouping: sizes, membership, rows ascending inside an aggregate
    bool grouped = (int32_t)g.ptr.size() == m + 1 && (int64_t)g.rows.size() == n && g.ptr[0] == 0;
    for (int32_t a = 0; grouped && a < m; ++a) {
        grouped = g.ptr[(size_t)a + 1] - g.ptr[(size_t)a] == sizes[(size_t)a];
        for (int32_t k = g.ptr[(size_t)a]; grouped && k < g.ptr[(size_t)a + 1]; ++k) {
            const int32_t r = g.rows[(size_t)k];
            grouped = r >= 0 && r < n && (int32_t)id[(size_t)r] - first_agg == a && (k == g.ptr[(size_t)a] || r > g.rows[(size_t)k - 1]);
        }
    }
    check("rows_grouped_by_aggregate_ascending", grouped, (double)n);
    // the pieces: every row of every aggregate in exactly one piece, none longer than the cap or empty, an aggregate's
    // pieces consecutive in table order and front to back
    std::vector<int> seen((size_t)n, 0);
    bool cover = (int32_t)g.piece_ptr.size() == m + 1 && g.piece_ptr[0] == 0 && g.piece_ptr[(size_t)m] == (int32_t)g.pieces.size();
    bool cap = true, consecutive = true;
    int32_t longest = 0, contiguous_aggregates = 0;
    for (size_t q = 0; q < g.pieces.size(); ++q) {
        const CoarsePiece &pc = g.pieces[q];
        if (pc.end - pc.begin > kCoarsePieceCap || pc.end <= pc.begin) cap = false;
        longest = std::max(longest, pc.end - pc.begin);
        if (pc.agg < 0 || pc.agg >= m) {
            cover = false;
            continue;
        }
        if (pc.begin < g.ptr[(size_t)pc.agg] || pc.end > g.ptr[(size_t)pc.agg + 1]) cover = false;
        if ((int32_t)q < g.piece_ptr[(size_t)pc.agg] || (int32_t)q >= g.piece_ptr[(size_t)pc.agg + 1]) consecutive = false;
        if (q > 0 && g.pieces[q - 1].agg > pc.agg) consecutive = false;
        if (q > 0 && g.pieces[q - 1].agg == pc.agg && g.pieces[q - 1].end != pc.begin) consecutive = false;
        for (int32_t k = std::max(pc.begin, 0); k < std::min<int32_t>(pc.end, (int32_t)n); ++k) ++seen[(size_t)g.rows[(size_t)k]];
    }
    for (int v : seen) cover = cover && v == 1;
    for (int32_t a = 0; a < m; ++a) {
        const int32_t want = (sizes[(size_t)a] + kCoarsePieceCap - 1) / kCoarsePieceCap;
        if (g.piece_ptr[(size_t)a + 1] - g.piece_ptr[(size_t)a] != want) consecutive = false;
        if (sizes[(size_t)a] > 1 && g.rows[(size_t)g.ptr[(size_t)a + 1] - 1] - g.rows[(size_t)g.ptr[(size_t)a]] == sizes[(size_t)a] - 1)
            ++contiguous_aggregates;
    }
    check("every_row_in_exactly_one_piece", cover, (double)n);
    check("no_piece_longer_than_the_cap", cap, (double)longest);
    check("pieces_of_an_aggregate_consecutive_in_table_order", consecutive, (double)g.pieces.size());
    std::printf("figure rows %" PRId64 " aggregates %d pieces %zu longest %d contiguous %d\n", n, m, g.pieces.size(), longest,
                contiguous_aggregates);
}

static void refusals()
{
    AggRows g;
    std::vector<CoarsePiece> pieces;
    std::vector<int32_t> piece_ptr;
    const uint16_t id[4] = {3, 4, 7, 3};
    const int32_t down[3] = {0, 5, 4}, late[2] = {1, 2};
    bool ok = group_rows_by_aggregate(4, id, 3, 2, &g) == SCHWZ_ERR_INVALID;      // id 7 outside [3, 5)
    ok = ok && group_rows_by_aggregate(4, id, 4, 4, &g) == SCHWZ_ERR_INVALID;      // id 3 below the range
    ok = ok && group_rows_by_aggregate(4, nullptr, 3, 5, &g) == SCHWZ_ERR_INVALID;
    ok = ok && group_rows_by_aggregate(4, id, 3, 5, nullptr) == SCHWZ_ERR_INVALID;
    ok = ok && plan_row_pieces(2, down, &pieces, &piece_ptr) == SCHWZ_ERR_INVALID;
    ok = ok && plan_row_pieces(1, late, &pieces, &piece_ptr) == SCHWZ_ERR_INVALID;
    ok = ok && plan_row_pieces(1, nullptr, &pieces, &piece_ptr) == SCHWZ_ERR_INVALID;
    ok = ok && group_rows_by_aggregate(4, id, 3, 5, &g) == SCHWZ_OK && g.ptr == std::vector<int32_t>({0, 2, 3, 3, 3, 4});
    ok = ok && group_rows_by_aggregate(0, nullptr, 0, 0, &g) == SCHWZ_OK && g.ptr == std::vector<int32_t>({0}) && g.rows.empty();
    ok = ok && plan_row_pieces(0, g.ptr.data(), &pieces, &piece_ptr) == SCHWZ_OK && pieces.empty() && piece_ptr == std::vector<int32_t>({0});
    check("bad_tables_are_refused_and_empty_ones_planned", ok, 0.0);
}

static const char *kCases[] = {"edge_sizes", "edge_sizes_first_agg_40", "one_long_aggregate", "empty_aggregates_only", "refusals"};

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: row_pieces_driver --list | <case>\n");
        return 2;
    }
    const std::string c = argv[1];
    const int32_t cap = kCoarsePieceCap;
    if (c == "--list") {
        for (const char *k : kCases) std::printf("%s\n", k);
        return 0;
    }
    if (c == kCases[0]) {
        run_case({0, 1, cap, cap + 1, 2 * cap + 1, 0, 2, 63, 64, 65, 255, 256, 257, cap - 1, 0}, 0);
    } else if (c == kCases[1]) {
        run_case({2 * cap + 1, 0, 1, cap + 1, cap}, 40);
    } else if (c == kCases[2]) {
        run_case({5 * cap + 7}, 0);
    } else if (c == kCases[3]) {
        run_case({0, 0, 0}, 2);
    } else if (c == kCases[4]) {
        refusals();
    } else {
        std::fprintf(stderr, "unknown case %s\n", c.c_str());
        return 2;
    }
    return failures ? 1 : 0;
}
