// The host plan of the aggregation coarse correction (csrc/coarse_plan.cpp) on the CPU, as a stand-alone program over
// coarse_plan.cpp and host_setup.cpp alone, built with the address and undefined-behaviour sanitizers
// (tests/test_coarse_plan.py runs it).  Per case it sets the subdomains up with the library's own host code, plans
// every subdomain and prints "check <name> pass|fail <figure>" per item and "digest <array> <hash>" per planned array.
//   coarse_plan_driver --list | <case>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "coarse_plan.hpp"

using namespace schwz;
typedef long double ld;

struct Global {
    int64_t N = 0;
    std::vector<int64_t> rp;
    std::vector<schwz_idx> col;
    std::vector<double> val;
    void add_row(const std::vector<std::pair<int64_t, double>> &e)
    {
        if (rp.empty()) rp.push_back(0);
        for (auto &x : e)
            if (x.second != 0.0) col.push_back((schwz_idx)x.first), val.push_back(x.second);
        rp.push_back((int64_t)col.size());
        ++N;
    }
};

// 7-point (nz > 1) or 5-point Laplacian, natural ordering, columns ascending; vary_diag: 0.5 + 0.001 (i % 5) added to the diagonal
static Global laplacian(int nx, int ny, int nz, bool vary_diag = false)
{
    Global g;
    const int dim = nz > 1 ? 3 : 2;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int64_t i = ((int64_t)z * ny + y) * nx + x;
                std::vector<std::pair<int64_t, double>> e;
                if (z > 0) e.push_back({i - (int64_t)nx * ny, -1.0});
                if (y > 0) e.push_back({i - nx, -1.0});
                if (x > 0) e.push_back({i - 1, -1.0});
                e.push_back({i, 2.0 * dim + (vary_diag ? 0.5 + 0.001 * (double)(i % 5) : 0.0)});
                if (x + 1 < nx) e.push_back({i + 1, -1.0});
                if (y + 1 < ny) e.push_back({i + nx, -1.0});
                if (z + 1 < nz) e.push_back({i + (int64_t)nx * ny, -1.0});
                g.add_row(e);
            }
    return g;
}

// 5-point diffusion plus first-order upwind convection on an n x n grid: kron(I, T) + kron(T, I) + 0.5 cx kron(I, D)
// - 0.5 cy kron(D^T, I) with T = tridiag(-1, 2, -1), D = bidiag(-1, 1) -- the generator of the suite's convdiff fixture
static Global convdiff(int n, double cx = 6.0, double cy = -3.0)
{
    Global g;
    for (int b = 0; b < n; ++b)
        for (int a = 0; a < n; ++a) {
            const int64_t i = (int64_t)b * n + a;
            std::vector<std::pair<int64_t, double>> e;
            if (b > 0) e.push_back({i - n, -1.0});
            if (a > 0) e.push_back({i - 1, -1.0 - 0.5 * cx});
            e.push_back({i, 4.0 + 0.5 * cx - 0.5 * cy});
            if (a + 1 < n) e.push_back({i + 1, -1.0});
            if (b + 1 < n) e.push_back({i + n, -1.0 + 0.5 * cy});
            g.add_row(e);
        }
    return g;
}

static Global neumann1d(int n)
{
    Global g;
    for (int i = 0; i < n; ++i) {
        std::vector<std::pair<int64_t, double>> e;
        if (i > 0) e.push_back({i - 1, -1.0});
        e.push_back({i, (i == 0 || i == n - 1) ? 1.0 : 2.0});
        if (i + 1 < n) e.push_back({i + 1, -1.0});
        g.add_row(e);
    }
    return g;
}

static uint64_t fnv(const void *p, size_t bytes, uint64_t h = 1469598103934665603ull)
{
    const unsigned char *c = (const unsigned char *)p;
    for (size_t k = 0; k < bytes; ++k) h = (h ^ c[k]) * 1099511628211ull;
    return h;
}

static int failures = 0;
static void check(const char *name, bool ok, double figure)
{
    std::printf("check %s %s %.3e\n", name, ok ? "pass" : "fail", figure);
    if (!ok) ++failures;
}

static double pseudo(int64_t i, int salt) { return std::sin(0.37 * (double)i + 1.3 * salt) + 0.25 * std::cos(0.011 * (double)i * i); }

// plans every subdomain of the case and checks it; agg: one id per global row (every id inside one subdomain, the
// ids of subdomain p a contiguous range, as the hosts number them)
static void run_case(const Global &g, int P, const std::vector<int32_t> &agg, bool expect_singular)
{
    const int64_t N = g.N;
    int32_t nc = 0;
    for (int32_t a : agg) nc = std::max(nc, a + 1);
    schwz_problem *prob = nullptr;
    if (schwz_problem_from_csr(N, g.rp.data(), g.col.data(), g.val.data(), &prob)) {
        std::printf("check problem fail 0\n%s\n", schwz_last_error());
        ++failures;
        return;
    }
    std::vector<int64_t> first_row((size_t)P + 1);
    schwz_partition_regular(N, P, first_row.data());
    std::vector<double> b((size_t)N), xg((size_t)N);
    for (int64_t i = 0; i < N; ++i) b[(size_t)i] = 1.0 + 0.01 * (double)(i % 7), xg[(size_t)i] = pseudo(i, 1);
    // brute force: Z^T (b - A x) and Z^T A Z in long double, with the sums of magnitudes the bounds are relative to
    std::vector<ld> s_ref((size_t)nc, 0), a0_ref((size_t)nc * nc, 0), a0_mag((size_t)nc * nc, 0);
    for (int64_t i = 0; i < N; ++i) {
        const int32_t a = agg[(size_t)i];
        s_ref[(size_t)a] += (ld)b[(size_t)i];
        for (int64_t k = g.rp[(size_t)i]; k < g.rp[(size_t)i + 1]; ++k) {
            const int64_t j = g.col[(size_t)k];
            s_ref[(size_t)a] -= (ld)g.val[(size_t)k] * (ld)xg[(size_t)j];
            a0_ref[(size_t)a * nc + agg[(size_t)j]] += (ld)g.val[(size_t)k];
            a0_mag[(size_t)a * nc + agg[(size_t)j]] += std::fabs((ld)g.val[(size_t)k]);
        }
    }
    std::vector<double> a0((size_t)nc * nc, 0.0);
    double worst_s = 0.0, worst_a0 = 0.0;
    bool cover = true, cap = true, ids = true;
    int64_t entries = 0, npieces = 0;
    uint64_t digest = 1469598103934665603ull;
    for (int me = 0; me < P; ++me) {
        schwz_subdomain *sd = nullptr;
        if (schwz_subdomain_setup(prob, P, me, 2, first_row.data(), &sd)) {
            std::printf("check setup fail %d\n%s\n", me, schwz_last_error());
            ++failures;
            continue;
        }
        const int64_t nloc = sd->local_size, nslots = sd->local_size_x + sd->halo_size;
        std::vector<int32_t> slot_agg((size_t)nslots);
        std::vector<double> xt((size_t)nslots), rhs((size_t)nloc);
        for (int64_t j = 0; j < nslots; ++j) slot_agg[(size_t)j] = agg[(size_t)sd->l2g[(size_t)j]], xt[(size_t)j] = xg[(size_t)sd->l2g[(size_t)j]];
        for (int64_t i = 0; i < nloc; ++i) rhs[(size_t)i] = b[(size_t)sd->l2g[(size_t)i]];
        int32_t first_agg = 0, m = 0;
        if (nloc > 0) {
            int32_t lo = nc, hi = -1;
            for (int64_t i = 0; i < nloc; ++i) lo = std::min(lo, slot_agg[(size_t)i]), hi = std::max(hi, slot_agg[(size_t)i]);
            first_agg = lo, m = hi - lo + 1;
        }
        CoarsePlan p;
        if (plan_coarse(nloc, nslots, sd->l_rp.data(), sd->l_col.data(), sd->l_val.data(), rhs.data(), slot_agg.data(), first_agg,
                        m, nc, &p)) {
            std::printf("check plan fail %d\n%s\n", me, schwz_last_error());
            ++failures;
            delete sd;  // (never on the device: nothing but host data)
            continue;
        }
        // beta - W x~ against the row-by-row sum
        for (int32_t a = 0; a < m; ++a) {
            double s = 0.0, mag = std::fabs(p.beta[(size_t)a]);
            for (int32_t k = p.w_ptr[(size_t)a]; k < p.w_ptr[(size_t)a + 1]; ++k) {
                s += p.w_val[(size_t)k] * xt[(size_t)p.w_slot[(size_t)k]];
                mag += std::fabs(p.w_val[(size_t)k] * xt[(size_t)p.w_slot[(size_t)k]]);
                if (k > p.w_ptr[(size_t)a] && p.w_slot[(size_t)k] <= p.w_slot[(size_t)k - 1]) ids = false;  // sorted by slot
                if (p.w_val[(size_t)k] == 0.0) ids = false;                                                  // zeros dropped
            }
            const double err = (double)std::fabs((ld)(p.beta[(size_t)a] - s) - s_ref[(size_t)(first_agg + a)]);
            worst_s = std::max(worst_s, err / (1e-13 * mag + 1e-300));
            for (int32_t c = 0; c < nc; ++c) {
                const double v = p.rows[(size_t)a * nc + c];
                a0[(size_t)(first_agg + a) * nc + c] = v;
                const double e2 = (double)std::fabs((ld)v - a0_ref[(size_t)(first_agg + a) * nc + c]);
                worst_a0 = std::max(worst_a0, e2 / (1e-13 * (double)a0_mag[(size_t)(first_agg + a) * nc + c] + 1e-300));
            }
        }
        // the pieces: every entry exactly once, aggregate after aggregate, none longer than the cap
        std::vector<int> seen(p.w_slot.size(), 0);
        for (size_t q = 0; q < p.pieces.size(); ++q) {
            const CoarsePiece &pc = p.pieces[q];
            if (pc.end - pc.begin > kCoarsePieceCap || pc.end <= pc.begin) cap = false;
            if (pc.agg < 0 || pc.agg >= m || pc.begin < p.w_ptr[(size_t)pc.agg] || pc.end > p.w_ptr[(size_t)pc.agg + 1]) cover = false;
            if ((int32_t)q < p.piece_ptr[(size_t)std::max(pc.agg, 0)] || (int32_t)q >= p.piece_ptr[(size_t)std::max(pc.agg, 0) + 1]) cover = false;
            for (int32_t k = std::max(pc.begin, 0); k < std::min<int32_t>(pc.end, (int32_t)seen.size()); ++k) ++seen[(size_t)k];
        }
        for (int v : seen) cover = cover && v == 1;
        for (int64_t j = 0; j < nslots; ++j) ids = ids && p.id16[(size_t)j] == (uint16_t)slot_agg[(size_t)j];
        entries += (int64_t)p.w_slot.size();
        npieces += (int64_t)p.pieces.size();
        digest = fnv(p.beta.data(), p.beta.size() * 8, digest);
        digest = fnv(p.w_ptr.data(), p.w_ptr.size() * 4, digest);
        digest = fnv(p.w_slot.data(), p.w_slot.size() * 4, digest);
        digest = fnv(p.w_val.data(), p.w_val.size() * 8, digest);
        digest = fnv(p.pieces.data(), p.pieces.size() * sizeof(CoarsePiece), digest);
        digest = fnv(p.piece_ptr.data(), p.piece_ptr.size() * 4, digest);
        digest = fnv(p.id16.data(), p.id16.size() * 2, digest);
        digest = fnv(p.rows.data(), p.rows.size() * 8, digest);
        delete sd;  // (never on the device: nothing but host data)
    }
    check("residual_equals_rowwise_sum", worst_s <= 1.0, worst_s * 1e-13);
    check("a0_rows_equal_brute_force", worst_a0 <= 1.0, worst_a0 * 1e-13);
    check("pieces_cover_every_entry_once", cover, (double)entries);
    check("no_piece_longer_than_the_cap", cap, (double)npieces);
    check("ids_sorted_zero_free_and_16_bit", ids, (double)nc);
    std::vector<double> inv((size_t)nc * nc);
    const int rc = schwz_dense_inverse(nc, a0.data(), inv.data());
    if (expect_singular) {
        const bool named = rc == SCHWZ_ERR_INVALID && std::strstr(schwz_last_error(), "singular") &&
                           std::strstr(schwz_last_error(), "Neumann") && std::strstr(schwz_last_error(), "aggregate");
        check("singular_a0_is_refused_with_its_cause", named, (double)rc);
    } else if (rc) {
        std::printf("check inverse fail %d\n%s\n", rc, schwz_last_error());
        ++failures;
    } else {
        double worst = 0.0, n1 = 0.0, n1i = 0.0;
        for (int32_t i = 0; i < nc; ++i)
            for (int32_t j = 0; j < nc; ++j) {
                ld s = 0;
                for (int32_t k = 0; k < nc; ++k) s += (ld)inv[(size_t)i * nc + k] * (ld)a0[(size_t)k * nc + j];
                worst = std::max(worst, (double)std::fabs(s - (i == j ? 1 : 0)));
            }
        for (int32_t j = 0; j < nc; ++j) {
            double c = 0.0, ci = 0.0;
            for (int32_t i = 0; i < nc; ++i) c += std::fabs(a0[(size_t)i * nc + j]), ci += std::fabs(inv[(size_t)i * nc + j]);
            n1 = std::max(n1, c), n1i = std::max(n1i, ci);
        }
        check("inverse_times_a0_is_identity", worst <= 1e-12, worst);
        std::printf("figure cond1_a0 %.3f\n", n1 * n1i);
        digest = fnv(inv.data(), inv.size() * 8, digest);
    }
    std::printf("figure nc %d entries %" PRId64 " pieces %" PRId64 "\n", nc, entries, npieces);
    std::printf("digest plan %016" PRIx64 "\n", digest);
    schwz_problem_destroy(prob);
}

static std::vector<int32_t> boxes(int nx, int ny, int nz, int bx, int by, int bz)
{
    // numbered z-layer of boxes after z-layer: with a partition into z-slabs the ids of a subdomain are a range
    std::vector<int32_t> agg((size_t)nx * ny * nz);
    const int cx = (nx + bx - 1) / bx, cy = (ny + by - 1) / by;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) agg[((size_t)z * ny + y) * nx + x] = ((z / bz) * cy + y / by) * cx + x / bx;
    return agg;
}

static const char *kCases[] = {"lap12_p3_boxes442", "lap16x10x7_p1_boxes454", "convdiff12_p3", "rows3_p5_empty_subdomains",
                               "shifted_lap64_two_aggregates", "neumann1d_singular"};

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: coarse_plan_driver --list | <case>\n");
        return 2;
    }
    const std::string c = argv[1];
    if (c == "--list") {
        for (const char *k : kCases) std::printf("%s\n", k);
        return 0;
    }
    if (c == kCases[0]) {
        run_case(laplacian(12, 12, 12), 3, boxes(12, 12, 12, 4, 4, 2), false);
    } else if (c == kCases[1]) {
        run_case(laplacian(16, 10, 7), 1, boxes(16, 10, 7, 4, 5, 4), false);
    } else if (c == kCases[2]) {
        std::vector<int32_t> agg(144);
        for (int i = 0; i < 144; ++i) agg[(size_t)i] = i / 8;  // 48 rows per subdomain: 6 aggregates of 8 rows each
        run_case(convdiff(12), 3, agg, false);
    } else if (c == kCases[3]) {
        Global g;
        g.add_row({{0, 2.0}, {1, -1.0}});
        g.add_row({{0, -1.0}, {1, 2.0}, {2, -1.0}});
        g.add_row({{1, -1.0}, {2, 2.0}});
        run_case(g, 5, {0, 1, 2}, false);
    } else if (c == kCases[4]) {
        // no column sum vanishes: W has an entry per slot, the first aggregate more than one piece
        std::vector<int32_t> agg(4096);
        for (int i = 0; i < 4096; ++i) agg[(size_t)i] = i < 4000 ? 0 : 1;
        run_case(laplacian(64, 64, 1, true), 1, agg, false);
    } else if (c == kCases[5]) {
        std::vector<int32_t> agg(12);
        for (int i = 0; i < 12; ++i) agg[(size_t)i] = i / 4;
        run_case(neumann1d(12), 1, agg, true);
    } else {
        std::fprintf(stderr, "unknown case %s\n", c.c_str());
        return 2;
    }
    return failures ? 1 : 0;
}
