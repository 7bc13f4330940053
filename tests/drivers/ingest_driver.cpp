// The ingest boundary of the host code (csrc/host_setup.cpp: the Matrix-Market reader, the problem sources from caller
// arrays, the first_row of a subdomain setup, the row checks of the factorizations, the graph partitioner on graphs that
// do not coarsen) on the CPU, as a stand-alone program over host_setup.cpp alone, built with the address and
// undefined-behaviour sanitizers (tests/test_ingest.py runs it).  A refusal prints "error <code> <message>"; an accepted
// problem prints N, then one line "row col value" per stored entry, the value as a hex float.
//   ingest_driver --list | file <path> | rows <path> | case <name>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "schwz_internal.hpp"

static void print_error(int rc) { std::printf("error %d %s\n", rc, schwz_last_error()); }

static int print_problem(const schwz_problem *p)
{
    std::printf("%" PRId64 "\n", p->N);
    std::vector<int64_t> c((size_t)p->max_row_nnz + 1);
    std::vector<double> v((size_t)p->max_row_nnz + 1);
    for (int64_t i = 0; i < p->N; ++i) {
        int len = 0;
        if (const int rc = schwz_problem_row(p, i, &len, c.data(), v.data(), p->max_row_nnz)) {
            print_error(rc);
            return 1;
        }
        for (int k = 0; k < len; ++k) std::printf("%" PRId64 " %" PRId64 " %a\n", i, c[(size_t)k], v[(size_t)k]);
    }
    return 0;
}

static uint64_t fnv(const void *p, size_t bytes, uint64_t h = 1469598103934665603ull)
{
    const unsigned char *c = (const unsigned char *)p;
    for (size_t k = 0; k < bytes; ++k) h = (h ^ c[k]) * 1099511628211ull;
    return h;
}

static int failures = 0;
static void check(const std::string &name, bool ok)
{
    std::printf("check %s %s\n", name.c_str(), ok ? "pass" : "fail");
    if (!ok) ++failures;
}

struct Csr {
    std::vector<int64_t> rp{0};
    std::vector<schwz_idx> col;
    std::vector<double> val;
    int64_t N() const { return (int64_t)rp.size() - 1; }
    void add_row(const std::vector<std::pair<int, double>> &e)
    {
        for (auto &x : e) col.push_back((schwz_idx)x.first), val.push_back(x.second);
        rp.push_back((int64_t)col.size());
    }
};

// ---- schwz_problem_from_csr --------------------------------------------------------------------------------------

static void from_csr(int64_t N, const std::vector<int64_t> &rp, const std::vector<schwz_idx> &col, const std::vector<double> &val)
{
    schwz_problem *p = nullptr;
    const int rc = schwz_problem_from_csr(N, rp.data(), col.data(), val.data(), &p);
    if (rc) {
        print_error(rc);
        return;
    }
    failures += print_problem(p);
    schwz_problem_destroy(p);
}

// ---- schwz_problem_from_rows: rows {1, 3, 4} of a 6 x 6 matrix -----------------------------------------------------

struct Rows {
    int64_t N = 6;
    std::vector<int64_t> ids{1, 3, 4}, rp{0, 2, 3, 5};
    std::vector<schwz_idx> col{0, 1, 3, 2, 4};
    std::vector<double> val{1.0, 2.0, 3.0, 4.0, 5.0};
    void run() const
    {
        schwz_problem *p = nullptr;
        const int rc = schwz_problem_from_rows(N, (int64_t)ids.size(), ids.data(), rp.data(), col.data(), val.data(), &p);
        if (rc) {
            print_error(rc);
            return;
        }
        std::printf("accepted %" PRId64 " rows\n", (int64_t)ids.size());
        schwz_problem_destroy(p);
    }
};

// ---- one file, P = 3, overlap 2: the subdomains of the whole problem and of the rows cut out for them ----------------

static bool same_subdomain(const schwz_subdomain *a, const schwz_subdomain *b)
{
    int64_t sa[10], sb[10];
    schwz_subdomain_sizes(a, sa);
    schwz_subdomain_sizes(b, sb);
    auto eq = [](const auto &x, const auto &y) {
        return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0);
    };
    bool ok = std::memcmp(sa, sb, sizeof(sa)) == 0;
    ok = ok && eq(a->l2g, b->l2g) && eq(a->l_rp, b->l_rp) && eq(a->l_col, b->l_col) && eq(a->l_val, b->l_val);
    ok = ok && eq(a->i_rp, b->i_rp) && eq(a->i_col_global, b->i_col_global) && eq(a->i_val, b->i_val);
    ok = ok && eq(a->nbr_in, b->nbr_in) && a->get.size() == b->get.size();
    for (size_t k = 0; ok && k < a->get.size(); ++k) ok = eq(a->get[k], b->get[k]);
    return ok;
}

static void rows_of_file(const char *path)
{
    const int P = 3, overlap = 2;
    schwz_problem *full = nullptr;
    if (const int rc = schwz_problem_from_matrix_market(path, &full)) {
        print_error(rc);
        ++failures;
        return;
    }
    std::vector<int64_t> first_row((size_t)P + 1);
    schwz_partition_regular(full->N, P, first_row.data());
    for (int me = 0; me < P; ++me) {
        schwz_subdomain *a = nullptr, *b = nullptr;
        schwz_problem *part = nullptr;
        int rc = schwz_subdomain_setup(full, P, me, overlap, first_row.data(), &a);
        std::vector<int64_t> ids, rp;
        std::vector<schwz_idx> col;
        std::vector<double> val;
        if (!rc) {
            // what the subdomain reads: its interior and overlap rows, ascending
            ids.assign(a->l2g.begin(), a->l2g.begin() + a->local_size_x);
            std::sort(ids.begin(), ids.end());
            rp.resize(ids.size() + 1);
            rc = schwz_problem_extract_rows(full, (int64_t)ids.size(), ids.data(), rp.data(), nullptr, nullptr);
        }
        if (!rc) {
            col.resize((size_t)rp.back());
            val.resize((size_t)rp.back());
            rc = schwz_problem_extract_rows(full, (int64_t)ids.size(), ids.data(), rp.data(), col.data(), val.data());
        }
        if (!rc) rc = schwz_problem_from_rows(full->N, (int64_t)ids.size(), ids.data(), rp.data(), col.data(), val.data(), &part);
        if (!rc) rc = schwz_subdomain_setup(part, P, me, overlap, first_row.data(), &b);
        if (rc) print_error(rc);
        check("subdomain_" + std::to_string(me) + "_same_on_extracted_rows", !rc && same_subdomain(a, b));
        if (a) std::printf("figure subdomain %d rows %" PRId64 " of %" PRId64 " local_nnz %" PRId64 "\n", me, (int64_t)ids.size(), full->N, (int64_t)a->l_col.size());
        delete a;  // (never on the device: nothing but host data)
        delete b;
        schwz_problem_destroy(part);
    }
    schwz_problem_destroy(full);
}

// ---- the row checks of the factorizations: a lower bidiagonal 3 x 3 matrix and four spoilt copies -----------------------

static void factor(const char *who, const char *what, const Csr &m)
{
    std::vector<schwz_idx> rp(m.rp.begin(), m.rp.end());
    schwz_idx *o[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double *lv = nullptr, *uv = nullptr, *w = nullptr;
    int rc;
    const int64_t n = (int64_t)rp.size() - 1;
    if (!std::strcmp(who, "cholesky"))
        rc = schwz_cholesky(n, rp.data(), m.col.data(), m.val.data(), 1, &o[0], &o[1], &lv, &o[2], &o[3], &uv, &o[4]);
    else if (!std::strcmp(who, "lu"))
        rc = schwz_lu(n, rp.data(), m.col.data(), m.val.data(), 1, &o[0], &o[1], &lv, &o[2], &o[3], &uv, &o[4], &o[5]);
    else
        rc = schwz_isai(n, rp.data(), m.col.data(), m.val.data(), 1, &w);
    std::printf("%s %s ", who, what);
    if (rc)
        print_error(rc);
    else
        std::printf("ok\n");
    for (schwz_idx *q : o) schwz_free(q);
    schwz_free(lv);
    schwz_free(uv);
    schwz_free(w);
}

// ---- schwz_partition_graph, schwz_problem_permute, schwz_subdomain_setup on graphs that do not coarsen -------------

static void partition(const Csr &m, int P)
{
    const int64_t N = m.N();
    schwz_problem *p = nullptr, *q = nullptr;
    if (const int rc = schwz_problem_from_csr(N, m.rp.data(), m.col.data(), m.val.data(), &p)) {
        print_error(rc);
        ++failures;
        return;
    }
    std::vector<uint32_t> part((size_t)N, 0xffffffffu);
    int rc = schwz_partition_graph(p, P, part.data());
    if (rc) print_error(rc);
    check("partition_graph_returns_ok", !rc);
    std::vector<int64_t> size((size_t)P, 0);
    bool ids = true;
    for (uint32_t id : part) {
        ids = ids && id < (uint32_t)P;
        if (id < (uint32_t)P) ++size[id];
    }
    check("every_id_below_P", ids);
    std::printf("sizes");
    for (int64_t s : size) std::printf(" %" PRId64, s);
    std::printf("\n");
    check("part_sizes_differ_by_at_most_one", *std::max_element(size.begin(), size.end()) - *std::min_element(size.begin(), size.end()) <= 1);
    std::vector<int64_t> perm((size_t)N), first_row((size_t)P + 1);
    rc = schwz_problem_permute(p, P, part.data(), perm.data(), first_row.data(), &q);
    if (rc) print_error(rc);
    check("permute_returns_ok", !rc);
    uint64_t digest = fnv(part.data(), part.size() * 4);
    int64_t total = 0;
    bool setups = !rc;
    for (int me = 0; !rc && me < P; ++me) {
        schwz_subdomain *sd = nullptr;
        if (const int rs = schwz_subdomain_setup(q, P, me, 2, first_row.data(), &sd)) {
            print_error(rs);
            setups = false;
            continue;
        }
        total += sd->local_size;
        setups = setups && sd->local_size == size[(size_t)me];
        digest = fnv(sd->l2g.data(), sd->l2g.size() * 8, digest);
        digest = fnv(sd->l_rp.data(), sd->l_rp.size() * 4, digest);
        digest = fnv(sd->l_col.data(), sd->l_col.size() * 4, digest);
        digest = fnv(sd->l_val.data(), sd->l_val.size() * 8, digest);
        digest = fnv(sd->i_col_global.data(), sd->i_col_global.size() * 8, digest);
        delete sd;  // (never on the device: nothing but host data)
    }
    check("every_subdomain_sets_up_with_its_part_size", setups);
    check("local_sizes_sum_to_N", total == N);
    digest = fnv(perm.data(), perm.size() * 8, digest);
    std::printf("digest partition %016" PRIx64 "\n", digest);
    schwz_problem_destroy(q);
    schwz_problem_destroy(p);
}

static const char *kCases[] = {"csr_row_ptr_starts_at_1",
                               "csr_row_ptr_not_monotone",
                               "csr_row_ptr_negative",
                               "csr_column_negative",
                               "csr_column_past_n",
                               "csr_unsorted_rows_are_sorted",
                               "csr_duplicates_are_summed_in_order",
                               "rows_accepts_its_base_case",
                               "rows_ids_not_ascending",
                               "rows_id_past_n",
                               "rows_columns_not_strictly_ascending",
                               "rows_column_past_n",
                               "rows_row_ptr_negative_at_every_position",
                               "rows_row_ptr_not_monotone_at_every_position",
                               "setup_first_row_decreases_or_runs_past_n",
                               "factor_rows_must_be_strictly_ascending",
                               "partition_diagonal3000_p7",
                               "partition_star3000_p7",
                               "partition_pairs1500_p7",
                               "partition_rows3_p8"};

static int run_case(const std::string &c)
{
    if (c == "csr_row_ptr_starts_at_1") {
        from_csr(2, {1, 2, 3}, {0, 0, 1}, {1.0, 2.0, 3.0});
    } else if (c == "csr_row_ptr_not_monotone") {
        from_csr(3, {0, 3, 1, 2}, {0, 1, 2}, {1.0, 2.0, 3.0});
    } else if (c == "csr_row_ptr_negative") {
        from_csr(2, {0, -2, -1}, {0}, {1.0});
    } else if (c == "csr_column_negative") {
        from_csr(2, {0, 1, 2}, {0, -1}, {1.0, 2.0});
    } else if (c == "csr_column_past_n") {
        from_csr(2, {0, 1, 2}, {0, 2}, {1.0, 2.0});
    } else if (c == "csr_unsorted_rows_are_sorted") {
        // the diagonal first, as deal.II stores it
        from_csr(3, {0, 2, 5, 7}, {0, 1, 1, 0, 2, 2, 1}, {4.0, -1.0, 4.5, -1.5, -2.0, 5.0, -2.5});
    } else if (c == "csr_duplicates_are_summed_in_order") {
        // column 1 of row 0: (1e16 + 1.0) + -1e16 = 0 in this order (1 in the other); column 0: 5 + 7
        from_csr(2, {0, 5, 6}, {1, 0, 1, 0, 1, 1}, {1e16, 5.0, 1.0, 7.0, -1e16, 2.0});
    } else if (c == "rows_accepts_its_base_case") {
        Rows().run();
    } else if (c == "rows_ids_not_ascending") {
        Rows r;
        r.ids = {1, 4, 3};
        r.run();
        r.ids = {1, 3, 3};
        r.run();
    } else if (c == "rows_id_past_n") {
        Rows r;
        r.ids = {1, 3, 6};
        r.run();
        r.ids = {-1, 3, 4};
        r.run();
    } else if (c == "rows_columns_not_strictly_ascending") {
        Rows r;
        r.col = {1, 0, 3, 2, 4};
        r.run();
        r.col = {0, 0, 3, 2, 4};
        r.run();
    } else if (c == "rows_column_past_n") {
        Rows r;
        r.col = {0, 1, 3, 2, 6};
        r.run();
        r.col = {-1, 1, 3, 2, 4};
        r.run();
    } else if (c == "rows_row_ptr_negative_at_every_position") {
        for (size_t k = 0; k < 4; ++k) {
            Rows r;
            r.rp[k] = -1;
            r.run();
        }
    } else if (c == "rows_row_ptr_not_monotone_at_every_position") {
        for (size_t k = 1; k < 3; ++k) {
            Rows r;
            r.rp[k] = r.rp[k + 1] + 1;
            r.run();
        }
    } else if (c == "setup_first_row_decreases_or_runs_past_n") {
        Csr m;
        for (int i = 0; i < 36; ++i) {
            std::vector<std::pair<int, double>> e;
            if (i > 0) e.push_back({i - 1, -1.0});
            e.push_back({i, 2.0});
            if (i < 35) e.push_back({i + 1, -1.0});
            m.add_row(e);
        }
        schwz_problem *p = nullptr;
        if (const int rc = schwz_problem_from_csr(36, m.rp.data(), m.col.data(), m.val.data(), &p)) {
            print_error(rc);
            return 1;
        }
        const int64_t bad[4][4] = {{0, 40, 20, 36}, {0, 20, 10, 36}, {0, -5, 20, 36}, {0, 12, 24, 40}};
        for (auto &fr : bad)
            for (int me = 0; me < 3; ++me) {
                schwz_subdomain *sd = nullptr;
                const int rc = schwz_subdomain_setup(p, 3, me, 2, fr, &sd);
                if (rc)
                    print_error(rc);
                else
                    std::printf("accepted\n");
                delete sd;
            }
        schwz_problem_destroy(p);
    } else if (c == "factor_rows_must_be_strictly_ascending") {
        Csr good, unsorted, twice, past, negative;
        good.add_row({{0, 2.0}}), good.add_row({{0, -1.0}, {1, 2.0}}), good.add_row({{1, -1.0}, {2, 2.0}});
        unsorted.add_row({{0, 2.0}}), unsorted.add_row({{1, 2.0}, {0, -1.0}}), unsorted.add_row({{1, -1.0}, {2, 2.0}});
        twice.add_row({{0, 2.0}}), twice.add_row({{0, -0.5}, {0, -0.5}, {1, 2.0}}), twice.add_row({{1, -1.0}, {2, 2.0}});
        past.add_row({{0, 2.0}}), past.add_row({{0, -1.0}, {1, 2.0}}), past.add_row({{1, -1.0}, {3, 2.0}});
        negative.add_row({{0, 2.0}}), negative.add_row({{-1, -1.0}, {1, 2.0}}), negative.add_row({{1, -1.0}, {2, 2.0}});
        for (const char *who : {"cholesky", "lu", "isai"}) {
            factor(who, "sorted", good);
            factor(who, "unsorted", unsorted);
            factor(who, "duplicate", twice);
            factor(who, "column_past_n", past);
            factor(who, "column_negative", negative);
        }
    } else if (c == "partition_diagonal3000_p7") {
        Csr m;
        for (int i = 0; i < 3000; ++i) m.add_row({{i, 1.0 + i}});
        partition(m, 7);
    } else if (c == "partition_star3000_p7") {
        Csr m;
        std::vector<std::pair<int, double>> hub;
        for (int i = 0; i < 3000; ++i) hub.push_back({i, i ? -1.0 : 3000.0});
        m.add_row(hub);
        for (int i = 1; i < 3000; ++i) m.add_row({{0, -1.0}, {i, 2.0}});
        partition(m, 7);
    } else if (c == "partition_pairs1500_p7") {
        Csr m;
        for (int i = 0; i < 3000; ++i) {
            if (i % 2 == 0)
                m.add_row({{i, 2.0}, {i + 1, -1.0}});
            else
                m.add_row({{i - 1, -1.0}, {i, 2.0}});
        }
        partition(m, 7);
    } else if (c == "partition_rows3_p8") {
        Csr m;
        m.add_row({{0, 2.0}, {1, -1.0}});
        m.add_row({{0, -1.0}, {1, 2.0}, {2, -1.0}});
        m.add_row({{1, -1.0}, {2, 2.0}});
        partition(m, 8);
    } else {
        std::fprintf(stderr, "unknown case %s\n", c.c_str());
        return 2;
    }
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc >= 2 ? argv[1] : "";
    if (argc == 2 && mode == "--list") {
        for (const char *k : kCases) std::printf("%s\n", k);
        return 0;
    }
    if (argc == 3 && mode == "file") {
        schwz_problem *p = nullptr;
        if (const int rc = schwz_problem_from_matrix_market(argv[2], &p)) {
            print_error(rc);
            return 0;
        }
        const int bad = print_problem(p);
        schwz_problem_destroy(p);
        return bad;
    }
    if (argc == 3 && mode == "rows") {
        rows_of_file(argv[2]);
        return failures ? 1 : 0;
    }
    if (argc == 3 && mode == "case") return run_case(argv[2]);
    std::fprintf(stderr, "usage: ingest_driver --list | file <path> | rows <path> | case <name>\n");
    return 2;
}
