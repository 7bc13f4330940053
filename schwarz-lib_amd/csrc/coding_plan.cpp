// Host-only planning of the matrix codings: see coding_plan.hpp.  No HIP runtime call, no environment read
// outside coding_options_from_env, no device query.
#include "coding_plan.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <unordered_map>

namespace schwz {

CodingOptions coding_options_from_env()
{
    // first character of a switch: '0' off, other digits as the field says, anything else the default (1)
    auto digit = [](const char *name, const char *known) {
        const char *e = std::getenv(name);
        return e && e[0] && std::strchr(known, e[0]) ? e[0] - '0' : 1;
    };
    auto number = [](const char *name) -> std::optional<int> {
        const char *e = std::getenv(name);
        return e ? std::optional<int>(std::atoi(e)) : std::nullopt;
    };
    CodingOptions o;
    o.pattern = digit("SCHWZ_SPMV_PATTERN", "02");
    o.pair = digit("SCHWZ_SPMV_PAIR", "023");
    o.dict = digit("SCHWZ_SPMV_DICT", "02");
    o.sym = digit("SCHWZ_SPMV_SYM", "0") != 0;
    o.rle = digit("SCHWZ_SPMV_RLE", "08");
    o.canon = digit("SCHWZ_SPMV_CANON", "0") != 0;
    o.sweep = number("SCHWZ_SPMV_SWEEP").value_or(1);
    o.sweep_gen = digit("SCHWZ_SWEEP_GEN", "0") != 0;
    o.sweep_T = number("SCHWZ_SWEEP_T");
    o.sweep_L = number("SCHWZ_SWEEP_L");
    o.sweep_Tdir = number("SCHWZ_SWEEP_TDIR");
    o.sweep_Ldir = number("SCHWZ_SWEEP_LDIR");
    o.sweep_first_per_cu = number("SCHWZ_SWEEP_FIRSTPERCU").value_or(6);
    // "u,d,f" per mille (update and start / fused direction / first direction table); one number: all three
    if (const char *e = std::getenv("SCHWZ_SWEEP_TRIM")) {
        int t[3] = {0, 0, 0}, n = 0;
        for (const char *c = e; n < 3; ++c) {
            t[n++] = std::atoi(c);
            if (!(c = std::strchr(c, ','))) break;
        }
        for (int k = n; k < 3; ++k) t[k] = n == 1 ? t[0] : 0;
        o.sweep_trim = t[0];
        o.sweep_trim_dir = t[1];
        o.sweep_trim_first = t[2];
    }
    o.sweep_cus = number("SCHWZ_SWEEP_CUS");
    const char *why = std::getenv("SCHWZ_SWEEP_WHY");
    o.sweep_why = why && why[0] == '1';
    return o;
}

namespace {

// FNV-1a over 64-bit words: the hash of every entry sequence and table that is de-duplicated here
constexpr uint64_t kFnvBasis = 1469598103934665603ull;
inline uint64_t fnv(uint64_t h, uint64_t x) { return (h ^ x) * 1099511628211ull; }

uint64_t fnv_entries(uint64_t h, const std::vector<PairEntryH> &seq)
{
    for (const PairEntryH &e : seq) h = fnv(fnv(fnv(fnv(h, e.va), e.vb), (uint64_t)(int64_t)e.off), (uint64_t)e.flags);
    return h;
}

// per-thread results of a parallel_blocks loop
template <typename T>
std::vector<T> per_thread(T init = T()) { return std::vector<T>((size_t)setup_threads(), init); }

struct RowPat {
    std::vector<uint64_t> bits;
    std::vector<schwz_idx> delta;
    bool operator==(const RowPat &o) const { return bits == o.bits && delta == o.delta; }
};

struct Table {
    int npat = 0, lmax = 0;
    std::vector<uint8_t> len;
    std::vector<double> val;       // [npat][lmax]
    std::vector<schwz_idx> delta;  // [npat][lmax]
    uint64_t hash = 0;
    bool same(const Table &o) const
    {
        return npat == o.npat && lmax == o.lmax && len == o.len && delta == o.delta &&
               std::memcmp(val.data(), o.val.data(), val.size() * sizeof(double)) == 0;
    }
};

// small open-addressing map from a 64-bit key to a code < 256, reset per tile
struct TinyMap {
    uint64_t key[512];
    int16_t code[512];
    int used[256];
    int n = 0;
    TinyMap() { std::memset(code, -1, sizeof(code)); }
    void reset()
    {
        for (int i = 0; i < n; ++i) code[used[i]] = -1;
        n = 0;
    }
    // returns the code, or -1 when a 257th distinct key arrives
    int get(uint64_t k)
    {
        uint64_t h = k * 0x9E3779B97F4A7C15ull;
        int slot = (int)(h >> 55);  // 9 bits
        while (code[slot] >= 0) {
            if (key[slot] == k) return code[slot];
            slot = (slot + 1) & 511;
        }
        if (n == kDictMax) return -1;
        key[slot] = k;
        code[slot] = (int16_t)n;
        used[n] = slot;
        return n++;
    }
};

// index of `x` in `list`, appended when new; -1 when that would be entry number `cap`
template <typename T>
int find_or_add(std::vector<T> &list, const T &x, int cap)
{
    for (size_t q = 0; q < list.size(); ++q)
        if (list[q] == x) return (int)q;
    if ((int)list.size() == cap) return -1;
    list.push_back(x);
    return (int)list.size() - 1;
}

// id of table `tb` among `tables` (equal tables share one), appended when new
template <typename T>
int share_table(std::vector<T> &tables, std::unordered_multimap<uint64_t, int> &by_hash, T &tb)
{
    auto range = by_hash.equal_range(tb.hash);
    for (auto it = range.first; it != range.second; ++it)
        if (tables[(size_t)it->second].same(tb)) return it->second;
    by_hash.emplace(tb.hash, (int)tables.size());
    tables.push_back(std::move(tb));
    return (int)tables.size() - 1;
}

}  // namespace

// The coding is accepted when it covers >= 90 % of the nonzeros and its tables are shared
// (SCHWZ_SPMV_PATTERN=0 disables, =2 forces whatever the coverage).
PatternPlan plan_patterns(const CodingOptions &opt, const HostCsr &M)
{
    PatternPlan P;
    const schwz_idx *rp = M.rp, *col = M.col;
    const std::vector<schwz_idx> &tiles = M.tiles;
    const int ntiles = (int)tiles.size() - 1;
    const int64_t nrows = tiles.back(), nnz = rp[nrows];
    if (opt.pattern == 0 || ntiles == 0 || nnz == 0) return P;
    P.pat_id.assign((size_t)nrows, 0);
    P.tile_table.assign((size_t)ntiles, -1);
    // every tile's table by all threads (a tile's rows, ids and table depend on that tile alone), then the tables
    // are de-duplicated in tile order -- the ids a sequential pass would give
    std::vector<Table> tile_tb((size_t)ntiles);
    std::vector<char> tile_ok((size_t)ntiles, 0);
    parallel_blocks(ntiles, 256, [&](int, int, int64_t t_begin, int64_t t_end) {
        std::vector<RowPat> pats;
        for (int t = (int)t_begin; t < (int)t_end; ++t) {
            const schwz_idx r0 = tiles[(size_t)t], r1 = tiles[(size_t)t + 1];
            if (rp[r1] == rp[r0] || (r1 - r0 == 1 && rp[r1] - rp[r0] > kTileNnz - 2)) continue;
            pats.clear();
            int lmax = 0;
            bool ok = true;
            RowPat p;
            for (schwz_idx r = r0; r < r1 && ok; ++r) {
                const int len = rp[r + 1] - rp[r];
                if (len > 255) {
                    ok = false;
                    break;
                }
                p.bits.resize((size_t)len);
                p.delta.resize((size_t)len);
                for (int k = 0; k < len; ++k) {
                    std::memcpy(&p.bits[(size_t)k], &M.val[rp[r] + k], 8);
                    p.delta[(size_t)k] = col[rp[r] + k] - r;
                }
                const int id = find_or_add(pats, p, kPatMax);
                if (id < 0) {
                    ok = false;
                    break;
                }
                if (id == (int)pats.size() - 1) lmax = std::max(lmax, len);
                P.pat_id[(size_t)r] = (uint8_t)id;
            }
            if (!ok || (int64_t)pats.size() * pat_stride(std::max(lmax, 1)) > kPatEntries) continue;
            Table &tb = tile_tb[(size_t)t];
            tb.npat = (int)pats.size();
            tb.lmax = std::max(lmax, 1);
            tb.len.resize((size_t)tb.npat);
            tb.val.assign((size_t)tb.npat * tb.lmax, 0.0);
            tb.delta.assign((size_t)tb.npat * tb.lmax, 0);
            uint64_t h = kFnvBasis;
            for (int q = 0; q < tb.npat; ++q) {
                tb.len[(size_t)q] = (uint8_t)pats[(size_t)q].bits.size();
                for (size_t k = 0; k < pats[(size_t)q].bits.size(); ++k) {
                    std::memcpy(&tb.val[(size_t)q * tb.lmax + k], &pats[(size_t)q].bits[k], 8);
                    tb.delta[(size_t)q * tb.lmax + k] = pats[(size_t)q].delta[k];
                    h = fnv(fnv(h, pats[(size_t)q].bits[k]), (uint64_t)(int64_t)pats[(size_t)q].delta[k]);
                }
                h = fnv(h, 0xffull ^ (uint64_t)tb.len[(size_t)q]);
            }
            tb.hash = h;
            tile_ok[(size_t)t] = 1;
        }
    });
    std::vector<Table> tables;
    std::unordered_multimap<uint64_t, int> by_hash;
    int64_t coded = 0;
    for (int t = 0; t < ntiles; ++t) {
        if (!tile_ok[(size_t)t]) continue;
        P.tile_table[(size_t)t] = share_table(tables, by_hash, tile_tb[(size_t)t]);
        coded += rp[tiles[(size_t)t + 1]] - rp[tiles[(size_t)t]];
    }
    tile_tb.clear();
    tile_tb.shrink_to_fit();
    P.fraction = (double)coded / (double)nnz;
    // a table pays off only when it is shared: with one table per tile the "coding" is just the
    // raw data in another layout
    if ((P.fraction < 0.9 || tables.size() * 4 > (size_t)ntiles) && opt.pattern != 2) return P;
    for (const Table &tb : tables) {
        P.tbl_desc.push_back((schwz_idx)P.tbl_val.size());
        P.tbl_desc.push_back((schwz_idx)P.tbl_len.size());
        P.tbl_desc.push_back(tb.npat);
        P.tbl_desc.push_back(tb.lmax);
        P.tbl_len.insert(P.tbl_len.end(), tb.len.begin(), tb.len.end());
        P.tbl_val.insert(P.tbl_val.end(), tb.val.begin(), tb.val.end());
        P.tbl_delta.insert(P.tbl_delta.end(), tb.delta.begin(), tb.delta.end());
    }
    P.built = true;
    return P;
}

// One thread, tile after tile: the dictionaries are concatenated in tile order, whatever the thread count.
DictPlan plan_dict(const CodingOptions &opt, const HostCsr &M, bool patterns_built)
{
    DictPlan P;
    const schwz_idx *rp = M.rp, *col = M.col;
    const int ntiles = (int)M.tiles.size() - 1;
    const int64_t nnz = rp[M.tiles.back()];
    // the row-pattern coding supersedes the per-entry one unless that is forced too
    if (opt.dict == 0 || (patterns_built && opt.dict != 2) || ntiles == 0 || nnz == 0) return P;
    P.code.assign((size_t)nnz, 0);
    P.vptr.assign((size_t)ntiles + 1, 0);
    P.dptr.assign((size_t)ntiles + 1, 0);
    std::vector<double> tv;
    std::vector<schwz_idx> td;
    TinyMap vm, dm;
    int64_t coded = 0;
    for (int t = 0; t < ntiles; ++t) {
        const schwz_idx r0 = M.tiles[(size_t)t], r1 = M.tiles[(size_t)t + 1];
        const int64_t s = rp[r0], e = rp[r1];
        // the kernel stages the codes of the 8-byte aligned window [s & ~3, e) : 2048 at most
        bool ok = e > s && (s & 3) + (e - s) <= kTileNnz;
        vm.reset();
        dm.reset();
        tv.clear();
        td.clear();
        for (schwz_idx r = r0; r < r1 && ok; ++r) {
            for (int64_t j = rp[r]; j < rp[r + 1]; ++j) {
                uint64_t bits;
                std::memcpy(&bits, &M.val[j], 8);
                const int before_v = vm.n, before_d = dm.n;
                const int cv = vm.get(bits);
                const int cdv = dm.get((uint64_t)(int64_t)(col[j] - r));
                if (cv < 0 || cdv < 0) {
                    ok = false;
                    break;
                }
                if (vm.n > before_v) tv.push_back(M.val[j]);
                if (dm.n > before_d) td.push_back(col[j] - r);
                P.code[(size_t)j] = (uint16_t)(cv | (cdv << 8));
            }
        }
        if (ok) {
            coded += e - s;
            P.vdict.insert(P.vdict.end(), tv.begin(), tv.end());
            P.ddict.insert(P.ddict.end(), td.begin(), td.end());
        }
        P.vptr[(size_t)t + 1] = (schwz_idx)P.vdict.size();
        P.dptr[(size_t)t + 1] = (schwz_idx)P.ddict.size();
    }
    P.fraction = (double)coded / (double)nnz;
    // worth it only when (nearly) the whole matrix is coded; SCHWZ_SPMV_DICT=2 forces it (tests)
    P.built = P.fraction >= 0.9 || opt.dict == 2;
    return P;
}

namespace {

// merged (offset, values, presence) sequence of the pair starting at row ra
void merge_pair(const HostCsr &M, int64_t ra, bool has_b, std::vector<PairEntryH> &cur)
{
    const schwz_idx *rp = M.rp, *col = M.col;
    cur.clear();
    schwz_idx ja = rp[ra], ea = rp[ra + 1];
    schwz_idx jb = has_b ? rp[ra + 1] : 0, eb = has_b ? rp[ra + 2] : 0;
    while (ja < ea || jb < eb) {
        const int64_t da = ja < ea ? (int64_t)col[ja] - ra : INT64_MAX;
        const int64_t db = jb < eb ? (int64_t)col[jb] - (ra + 1) : INT64_MAX;
        PairEntryH e = {0, 0, 0, 0};
        const int64_t d = std::min(da, db);
        e.off = (schwz_idx)d;
        if (da == d) {
            e.flags |= 1;
            std::memcpy(&e.va, &M.val[ja], 8);
            ++ja;
        }
        if (db == d) {
            e.flags |= 2;
            std::memcpy(&e.vb, &M.val[jb], 8);
            ++jb;
        }
        cur.push_back(e);
    }
}

// rows [r0, r1) can be pair coded: at most 127 entries each, strictly ascending columns (merged order == each
// row's order needs sorted rows)
bool rows_codable(const HostCsr &M, int64_t r0, int64_t r1)
{
    for (int64_t r = r0; r < r1; ++r) {
        if (M.rp[r + 1] - M.rp[r] > 127) return false;
        for (schwz_idx j = M.rp[r] + 1; j < M.rp[r + 1]; ++j)
            if (M.col[j] <= M.col[j - 1]) return false;
    }
    return true;
}

PairTable table_from_patterns(const std::vector<std::vector<PairEntryH>> &pats, int lmax)
{
    PairTable tb;
    tb.npat = (int)pats.size();
    tb.lmax = lmax;
    tb.len.resize((size_t)tb.npat);
    tb.ent.assign((size_t)tb.npat * lmax, PairEntryH{0, 0, 0, 0});
    tb.hash = kFnvBasis;
    for (int q = 0; q < tb.npat; ++q) {
        tb.len[(size_t)q] = (uint8_t)pats[(size_t)q].size();
        std::copy(pats[(size_t)q].begin(), pats[(size_t)q].end(), tb.ent.begin() + (size_t)q * lmax);
        tb.hash = fnv(fnv_entries(tb.hash, pats[(size_t)q]), 0xffull ^ (uint64_t)tb.len[(size_t)q]);
    }
    return tb;
}

// the entries on and above the diagonal only, the strictly upper ones doubled (exact)
PairTable upper_twin(const PairTable &src)
{
    PairTable u;
    u.npat = src.npat;
    u.len.assign((size_t)u.npat, 0);
    u.lmax = 1;
    for (int q = 0; q < src.npat; ++q) {
        int cnt = 0;
        for (int k = 0; k < (int)src.len[(size_t)q]; ++k) cnt += src.ent[(size_t)q * src.lmax + k].off >= 0;
        u.len[(size_t)q] = (uint8_t)cnt;
        u.lmax = std::max(u.lmax, cnt);
    }
    u.ent.assign((size_t)u.npat * u.lmax, PairEntryH{0, 0, 0, 0});
    for (int q = 0; q < src.npat; ++q) {
        int w = 0;
        for (int k = 0; k < (int)src.len[(size_t)q]; ++k) {
            PairEntryH e = src.ent[(size_t)q * src.lmax + k];
            if (e.off < 0) continue;
            if (e.off > 0) {
                double va, vb;
                std::memcpy(&va, &e.va, 8);
                std::memcpy(&vb, &e.vb, 8);
                va *= 2.0;
                vb *= 2.0;
                std::memcpy(&e.va, &va, 8);
                std::memcpy(&e.vb, &vb, 8);
            }
            u.ent[(size_t)q * u.lmax + w++] = e;
        }
    }
    return u;
}

// ONE table for the whole matrix (a constant-coefficient stencil has a few dozen distinct pairs in total); the
// kernel then stages it once and looks nothing up per chunk.  false: the matrix has no such table.
bool single_table(const HostCsr &M, PairPlan &P)
{
    const int64_t nrows = M.tiles.back();
    std::vector<char> unsorted = per_thread<char>();
    parallel_blocks(nrows, 1 << 16, [&](int t, int, int64_t a, int64_t b) { unsorted[(size_t)t] = !rows_codable(M, a, b); });
    if (std::find(unsorted.begin(), unsorted.end(), 1) != unsorted.end()) return false;
    // Every thread codes a contiguous block of pairs against a dictionary of its own (ids in ITS order of
    // first appearance); the dictionaries are then merged in block order, which numbers the patterns in
    // the order a sequential pass meets them, and the ids are renumbered.
    const int64_t npairs = (nrows + 1) / 2;
    auto tpats = per_thread<std::vector<std::vector<PairEntryH>>>();
    std::vector<char> tfail = per_thread<char>();
    const int nthreads = parallel_blocks(npairs, 1 << 15, [&](int t, int, int64_t a, int64_t b) {
        auto &mine = tpats[(size_t)t];
        std::unordered_multimap<uint64_t, int> seen;
        std::vector<PairEntryH> cur;
        for (int64_t pi = a; pi < b; ++pi) {
            merge_pair(M, 2 * pi, 2 * pi + 1 < nrows, cur);
            const uint64_t h = fnv_entries(kFnvBasis, cur);
            int id = -1;
            auto range = seen.equal_range(h);
            for (auto it = range.first; it != range.second; ++it)
                if (mine[(size_t)it->second] == cur) {
                    id = it->second;
                    break;
                }
            if (id < 0) {
                id = (int)mine.size();
                if (id == kPairPats) {
                    tfail[(size_t)t] = 1;
                    break;
                }
                seen.emplace(h, id);
                mine.push_back(cur);
            }
            P.pair_id[(size_t)pi] = (uint8_t)id;
        }
    });
    std::vector<std::vector<PairEntryH>> pats;
    std::vector<std::vector<int>> remap((size_t)nthreads);
    int lmax = 1;
    for (int t = 0; t < nthreads; ++t) {
        if (tfail[(size_t)t]) return false;
        for (const auto &pt : tpats[(size_t)t]) {
            const int id = find_or_add(pats, pt, kPairPats);
            if (id == (int)pats.size() - 1) lmax = std::max(lmax, (int)pt.size());
            if (id < 0 || (int64_t)pats.size() * pair_stride(lmax) > kPairEntries) return false;
            remap[(size_t)t].push_back(id);
        }
    }
    // the same blocks again (parallel_blocks cuts [0, npairs) the same way for the same n and grain)
    parallel_blocks(npairs, 1 << 15, [&](int t, int, int64_t a, int64_t b) {
        const auto &mp = remap[(size_t)t];
        for (int64_t pi = a; pi < b; ++pi) P.pair_id[(size_t)pi] = (uint8_t)mp[(size_t)P.pair_id[(size_t)pi]];
    });
    P.tables.push_back(table_from_patterns(pats, lmax));
    std::fill(P.chunk_ptable.begin(), P.chunk_ptable.end(), 0);
    return true;
}

// A table per chunk of 512 rows, equal tables shared; returns the nonzeros in coded chunks.
int64_t chunk_tables(const HostCsr &M, PairPlan &P)
{
    const int64_t nrows = M.tiles.back();
    std::unordered_multimap<uint64_t, int> by_hash;
    std::vector<std::vector<PairEntryH>> pats;
    std::vector<PairEntryH> cur;
    int64_t coded = 0;
    for (size_t c = 0; c < P.chunk_ptable.size(); ++c) {
        const int64_t r0 = (int64_t)c * kPairRows, r1 = std::min<int64_t>(r0 + kPairRows, nrows);
        if (M.rp[r1] == M.rp[r0] || !rows_codable(M, r0, r1)) continue;
        pats.clear();
        int lmax = 1;
        bool ok = true;
        for (int64_t ra = r0; ra < r1 && ok; ra += 2) {
            merge_pair(M, ra, ra + 1 < r1, cur);
            const int id = find_or_add(pats, cur, kPairPats);
            if (id < 0) {
                ok = false;
                break;
            }
            if (id == (int)pats.size() - 1) lmax = std::max(lmax, (int)cur.size());
            P.pair_id[(size_t)(ra >> 1)] = (uint8_t)id;
        }
        if (!ok || (int64_t)pats.size() * pair_stride(lmax) > kPairEntries) continue;
        PairTable tb = table_from_patterns(pats, lmax);
        P.chunk_ptable[c] = share_table(P.tables, by_hash, tb);
        coded += M.rp[r1] - M.rp[r0];
    }
    return coded;
}

// run-length form of the ids: R x (first pair of the run | id << 8) per chunk, 0xffff first: more than R runs
std::vector<uint16_t> rle_records(const PairPlan &P, int64_t nrows, int R, int64_t *coded_out)
{
    const int64_t nchunks = (int64_t)P.chunk_ptable.size();
    std::vector<uint16_t> out((size_t)nchunks * R, 0xffffu);
    std::vector<int64_t> coded_t = per_thread<int64_t>();
    parallel_blocks(nchunks, 2048, [&](int t, int, int64_t c_begin, int64_t c_end) {
        int64_t mine = 0;
        for (int64_t c = c_begin; c < c_end; ++c) {
            if (P.chunk_ptable[(size_t)c] < 0) continue;
            const int64_t p0 = c * (kPairRows / 2), p1 = std::min<int64_t>(p0 + kPairRows / 2, (nrows + 1) / 2);
            uint16_t runs[16];
            int nr = 0;
            bool fits = true;
            for (int64_t p = p0; p < p1 && fits; ++p) {
                if (nr == 0 || P.pair_id[(size_t)p] != (uint8_t)(runs[nr - 1] >> 8)) {
                    if (nr == R) {
                        fits = false;
                        break;
                    }
                    runs[nr++] = (uint16_t)((p - p0) | ((int)P.pair_id[(size_t)p] << 8));
                }
            }
            if (!fits || nr == 0) continue;
            for (int k = nr; k < R; ++k) runs[k] = runs[nr - 1];
            if (runs[0] == 0xffffu) continue;  // would read as the "not coded" marker
            std::copy(runs, runs + R, out.begin() + (size_t)c * R);
            ++mine;
        }
        coded_t[(size_t)t] = mine;
    });
    *coded_out = 0;
    for (int64_t v : coded_t) *coded_out += v;
    return out;
}

}  // namespace

// Accepted when >= 90 % of the nonzeros sit in pair-coded chunks and the tables are shared
// (SCHWZ_SPMV_PAIR=0 disables, =2 forces whatever the coverage, =3: per-chunk tables even if one would do).
bool plan_pair_tables(const CodingOptions &opt, const HostCsr &M, PairPlan &P)
{
    if (opt.pair == 0 || M.tiles.size() < 2) return false;
    const int64_t nrows = M.tiles.back(), nnz = M.rp[nrows];
    if (nnz == 0 || M.ncols < 2 || M.ncols >= INT32_MAX || nrows >= INT32_MAX - kPairRows) return false;
    const size_t nchunks = (size_t)((nrows + kPairRows - 1) / kPairRows);
    P.pair_id.assign((size_t)(nrows + 1) / 2, 0);
    P.chunk_ptable.assign(nchunks, -1);
    {
        StageTimer t_single("  pairs: one table for the whole matrix");
        P.single = opt.pair != 3 && single_table(M, P);
    }
    P.fraction = (double)(P.single ? nnz : chunk_tables(M, P)) / (double)nnz;
    const bool force = opt.pair == 2;
    if (P.fraction < 0.9 && !force) return false;
    if (!P.single && P.tables.size() * 4 > nchunks && !force) return false;  // tables must be shared to pay off
    // Symmetric matrix (checked bit for bit): a second set of tables with the entries on and above the
    // diagonal only, for kSpmvDotSym.  SCHWZ_SPMV_SYM=0 skips it.
    StageTimer t_sym("  pairs: symmetry check, upper-triangle twins");
    if (opt.sym && csr_is_symmetric(nrows, M.ncols, M.rp, M.col, M.val)) {
        P.sym_base = (int)P.tables.size();
        for (int t = 0; t < P.sym_base; ++t) P.tables.push_back(upper_twin(P.tables[(size_t)t]));
    }
    return P.built = true;
}

void plan_pair_records(const CodingOptions &opt, const HostCsr &M, int deal_shift, PairPlan &P)
{
    const int64_t nrows = M.tiles.back();
    for (const PairTable &tb : P.tables) {
        P.ptbl_desc.push_back((schwz_idx)(P.ptbl_val.size() / 2));
        P.ptbl_desc.push_back((schwz_idx)P.ptbl_len.size());
        P.ptbl_desc.push_back(tb.npat);
        P.ptbl_desc.push_back(tb.lmax);
        schwz_idx reach = 0;
        for (const PairEntryH &e : tb.ent) reach = std::max<schwz_idx>(reach, e.off < 0 ? -e.off : e.off);
        P.ptbl_desc.push_back(reach);
        P.ptbl_len.insert(P.ptbl_len.end(), tb.len.begin(), tb.len.end());
        for (const PairEntryH &e : tb.ent) {
            double va, vb;
            std::memcpy(&va, &e.va, 8);
            std::memcpy(&vb, &e.vb, 8);
            P.ptbl_val.push_back(va);
            P.ptbl_val.push_back(vb);
            P.ptbl_meta.push_back(e.off);
            P.ptbl_meta.push_back(e.flags);
        }
    }
    // run-length form of the ids, chunk by chunk (SCHWZ_SPMV_RLE=0: byte ids only)
    // Records of 8 runs (16 bytes per chunk) serve x lines of ~170 entries and more; a matrix some of whose
    // chunks need up to 16 runs (a 512-row chunk of a 192 x 192 plane crosses three line ends: ten runs) gets
    // records of 16 runs (32 bytes per chunk) throughout -- SCHWZ_SPMV_RLE=8 keeps the short records.
    if (opt.rle != 0) {
        int64_t coded8 = 0, coded16 = 0;
        P.rle = rle_records(P, nrows, 8, &coded8);
        if (opt.rle != 8) {
            std::vector<uint16_t> wide = rle_records(P, nrows, 16, &coded16);
            if (coded16 > coded8) {
                P.rle.swap(wide);
                P.rle_runs = 16;
            }
        }
    }
    // canonical stencil layout of a single-table matrix (SCHWZ_SPMV_CANON=0: off): the offsets of its
    // commonest pattern when they read {<= 2 below -1, -1, 0, +1, <= 2 above +1}; missing outer slots
    // repeat their neighbour outwards, so an entry always lands in the lowest slot with its offset and
    // the slots stay in ascending entry order
    if (P.single && opt.canon) {
        const PairTable &tb = P.tables[0];
        std::vector<int64_t> freq((size_t)tb.npat, 0);
        for (uint8_t id : P.pair_id) ++freq[(size_t)id];
        const int best = (int)(std::max_element(freq.begin(), freq.end()) - freq.begin());
        std::vector<schwz_idx> neg, pos;
        bool has_m1 = false, has_0 = false, has_p1 = false;
        for (int k = 0; k < (int)tb.len[(size_t)best]; ++k) {
            const schwz_idx off = tb.ent[(size_t)best * tb.lmax + k].off;
            if (off == -1) has_m1 = true;
            else if (off == 0) has_0 = true;
            else if (off == 1) has_p1 = true;
            else if (off < 0) neg.push_back(off);
            else pos.push_back(off);
        }
        if (has_m1 && has_0 && has_p1 && neg.size() <= 2 && pos.size() <= 2) {
            std::sort(neg.begin(), neg.end());  // most negative first
            std::sort(pos.begin(), pos.end());
            const schwz_idx n2 = neg.size() >= 1 ? neg[0] : -1;
            const schwz_idx n1 = neg.size() == 2 ? neg[1] : n2;
            const schwz_idx p2 = pos.size() >= 1 ? pos.back() : 1;
            const schwz_idx p1 = pos.size() == 2 ? pos[0] : p2;
            const schwz_idx lay[8] = {n2, n1, -1, 0, 1, p1, p2, 1};
            std::copy(lay, lay + 8, P.canon);
        }
    }
    // what a pass over the coded matrix reads: per chunk its 16-byte run-length record, or one byte per
    // pair where the ids do not run-length code; the chunk's table id unless one table serves the whole
    // matrix; the tables themselves (one set; the upper-triangle twins are read INSTEAD by kSpmvDotSym)
    for (size_t c = 0; c < P.chunk_ptable.size(); ++c) {
        if (P.chunk_ptable[c] < 0) continue;
        const bool has_rle = !P.rle.empty(), runs = has_rle && P.rle[c * P.rle_runs] != 0xffffu;
        P.code_bytes += runs ? 2 * P.rle_runs : (has_rle ? 2 * P.rle_runs : 0) + kPairRows / 2;
        if (!P.single) P.code_bytes += 4;
    }
    const size_t ntab = P.sym_base ? (size_t)P.sym_base : P.tables.size();
    for (size_t t = 0; t < ntab; ++t) P.code_bytes += (int64_t)P.tables[t].ent.size() * 24 + P.tables[t].npat;
    // the XCD deal of the chunks: the tile deal's run length in rows, in chunks (a power of two)
    P.shift = deal_shift;
    const int64_t rows_per_tile = std::max<int64_t>(1, nrows / std::max<int64_t>(1, (int64_t)M.tiles.size() - 1));
    for (int64_t f = kPairRows / std::max<int64_t>(1, rows_per_tile); f > 1 && P.shift > 0; f >>= 1) --P.shift;
}

namespace {

using Run = WalkRun;  // chain positions [p0, p1) of consecutive walkable planes

// segments a launch needs when its runs are cut into pieces of at most `len` chain positions, per band
int64_t segment_count(const std::vector<Run> &runs, int bands, int len)
{
    int64_t n = 0;
    for (const Run &r : runs) n += (int64_t)((r.p1 - r.p0 + len - 1) / len) * bands;
    return n;
}

// Segment length of a launch on bands of T rows: `asked` (SCHWZ_SWEEP_L / LDIR), else about wg_per_cu
// segments per CU in ONE round of workgroups, at least `floor` positions.  (Below 2 only when asked: 16.)
int segment_length(const std::vector<Run> &runs, int64_t PL, int T, std::optional<int> asked, int wg_per_cu, int cus, int floor)
{
    const int bands = (int)((PL + T - 1) / T);
    int64_t steps = 0;
    for (const Run &r : runs) steps += (int64_t)(r.p1 - r.p0) * bands;
    const int64_t wgs = (int64_t)wg_per_cu * cus;
    const int L = asked ? *asked : (int)std::max<int64_t>(floor, (steps + wgs - 1) / wgs);
    return L < 2 ? 16 : L;
}

}  // namespace

// (coding_plan.hpp)
std::vector<int4> walk_segment_table(const std::vector<WalkRun> &runs, int64_t PL, int T, int L, int cus, int trim,
                                     int floor, int step, int room)
{
    const int bands = (int)((PL + T - 1) / T);  // (gen mode: the last band of a plane is partial)
    while (segment_count(runs, bands, L) + kXcds > room && L < (1 << 20)) L += step;
    trim = std::min(std::max(trim, 0), kWalkTrimMax);
    // equal pieces of `len` positions are ceil(R / len) pieces: nseg of them, or one less where the remainder is nothing
    auto pieces = [&](const Run &r, int &len) {
        const int R = r.p1 - r.p0, nseg = (R + L - 1) / L;
        len = (R + nseg - 1) / nseg;
        return (R + len - 1) / len;
    };
    int64_t filled = 0, late_left = 0;
    for (const Run &r : runs) {
        int len;
        filled += (int64_t)pieces(r, len) * bands;
    }
    // Pieces from the end of the table that are late: piece j from the end holds the sorted entries
    // [filled - (j + 1) bands, filled - j bands), of which min(bands, cus - j bands) are among the last `cus`.
    if (trim > 0 && filled > cus)
        for (int64_t j = 0; 2 * std::min<int64_t>(bands, (int64_t)cus - j * bands) > bands; ++j) late_left = j + 1;
    struct Seg { int band, p0, p1; };
    std::vector<Seg> segs;
    std::vector<std::vector<int>> cuts(runs.size());  // per run: the first position of every piece, and p1
    for (size_t i = runs.size(); i-- > 0;) {
        const Run &r = runs[i];
        int len;
        const int R = r.p1 - r.p0, npieces = pieces(r, len);
        std::vector<int> &c = cuts[i];
        const int late = (int)std::min<int64_t>(late_left, npieces), early = npieces - late;
        late_left -= late;
        if (late == 0 || early == 0 || len < kWalkTrimMinLen) {
            // equal pieces, the last one the remainder: what every table was before there was a trim
            for (int p = r.p0; p < r.p1; p += len) c.push_back(p);
        } else {
            // early e, late (1 - t) e, early e + late (1 - t) e = R; whole positions: the late pieces' share rounded to
            // the nearest, lowered until no late piece is longer than an early one, never below the floor
            const double keep = 1.0 - trim / 1000.0;
            int late_sum = (int)(late * keep * R / (early + late * keep) + 0.5);
            while (late_sum > late && (late_sum + late - 1) / late > (R - late_sum) / early) --late_sum;
            late_sum = std::max(late_sum, late * std::min(floor, len));
            const int early_sum = R - late_sum;
            int p = r.p0;
            for (int k = 0; k < early; ++k) {
                c.push_back(p);
                p += early_sum / early + (k < early_sum % early ? 1 : 0);
            }
            for (int k = 0; k < late; ++k) {
                c.push_back(p);
                p += late_sum / late + (k < late_sum % late ? 1 : 0);
            }
        }
        c.push_back(r.p1);
    }
    for (size_t i = 0; i < runs.size(); ++i)
        for (int b = 0; b < bands; ++b)
            for (size_t k = 0; k + 1 < cuts[i].size(); ++k) segs.push_back({b, cuts[i][k], cuts[i][k + 1]});
    // deal: XCD x takes the bands [x * bands / 8, (x + 1) * bands / 8) (a band's window shares its NX-row
    // halos with the neighbouring bands: the same L2), segment by segment along the chain
    std::stable_sort(segs.begin(), segs.end(), [](const Seg &x, const Seg &y) { return x.p0 != y.p0 ? x.p0 < y.p0 : x.band < y.band; });
    std::vector<std::vector<int4>> per_xcd(kXcds);
    for (const Seg &sgm : segs) {
        int4 v;
        v.x = sgm.band;
        v.y = sgm.p0;
        v.z = sgm.p1;
        v.w = (int)std::min<int64_t>(T, PL - (int64_t)sgm.band * T);  // rows of the band inside the plane
        size_t x;
        if (bands >= 2 * kXcds) {
            x = (size_t)((int64_t)sgm.band * kXcds / bands);
        } else {  // few bands: round robin
            x = 0;
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

// The z-sweep walk (spmv_pair_sweep_kernel, spmv_pair_dirdot_sweep_kernel): host side.
//
// Geometry.  The matrix is cut into PLANES of PL consecutive rows (PL = the dominant far offset of the
// canonical layout, NX its in-plane line offset).  A row of plane k may couple to {-NX, -1, 0, +1, +NX}
// inside its plane and to the row at the SAME in-plane position of at most two other planes: for the
// interior of a grid in natural order those are k - 1 and k + 1; for a subdomain whose overlap planes are
// appended behind its interior the first interior plane couples to the plane PL rows on and
// to the lower overlap plane far behind it, and so on.  Planes linked like that form CHAINS; a workgroup
// sweeps a band of rows along a chain and keeps the windows of three consecutive chain positions in LDS,
// so every far operand of a row is in the window before or after its own -- wherever the numbering put
// that plane.  Slots of a row pair, in the order the entries are summed (= ascending column, the CSR
// order): [far before 0, far before 1, -NX, -1, 0, +1, +NX, far after 0, far after 1]; which window
// (previous / next chain position) a far slot reads is a property of the plane (chain_far).
// A plane takes part when all its chunks are full, run-length coded, and every pattern in them fits those
// slots; the rest of the matrix is left to the companion launch (gen).
WalkPlan plan_walk(const CodingOptions &opt, const PairPlan &P, int64_t nrows, int64_t ncols, int grid, int cus,
                   int dirdot_halo_lines)
{
    WalkPlan W;
    if (!P.single) return W;
    if (opt.sweep_cus && *opt.sweep_cus > 0) cus = *opt.sweep_cus;  // SCHWZ_SWEEP_CUS: planned for another CU count
    auto no_walk = [&](const char *why) {
        W = WalkPlan();
        W.why = why;
        return W;
    };
    const PairTable &tb = P.tables[0];
    const PairTable *ts = P.sym_base > 0 ? &P.tables[(size_t)P.sym_base] : nullptr;
    const std::vector<uint16_t> &rle = P.rle;
    const int *cn = P.canon;
    // A 5-point (2-D) stencil {-N, -1, 0, +1, +N} in natural order is the same walk with the x LINE in the role of the
    // plane: the canonical layout then repeats its outer offsets (cn[0] == cn[1] == -N, cn[5] == cn[6] == N), the
    // +-N neighbours sit at the same position of the previous / next line (the far slots), and nothing couples rows
    // +-NX apart inside a "plane" -- NX is only the width of the halo the kernels load around a band, 2 rows: the
    // band's left and right neighbour.
    const bool two_d = cn[7] && cn[5] == cn[6] && cn[0] == cn[1] && cn[6] > 2;
    const int64_t NX = two_d ? 2 : cn[5], PL = cn[6];
    // Planes of whole 512-row chunks: a band's sub-bands ARE chunks and the pattern ids come from the chunk's
    // run-length record.  Any other even plane size (200 x 200, 300 x 300, ...; round 3): "gen mode" -- byte ids, a
    // partial last band per plane, and the walk must cover the whole matrix (no companion launch: its unit is the
    // chunk, and chunks straddle planes there).  SCHWZ_SWEEP_GEN=0: whole-chunk planes only.
    const bool gen_mode = PL % kPairRows != 0;
    const bool shape_ok = cn[7] && cn[0] == -PL && (two_d || cn[1] == -NX) && NX >= 2 && PL > NX && NX % 2 == 0 && PL % 2 == 0 &&
                          NX <= 1024 && (!gen_mode || (opt.sweep_gen && nrows % PL == 0 && PL >= kPairRows));
    if (opt.sweep == 0) return no_walk("switched off (SCHWZ_SPMV_SWEEP=0)");
    if (!cn[7]) return no_walk("no canonical stencil layout (the patterns do not share one set of offsets)");
    if (!shape_ok) return no_walk("offsets are not those of an x-y-z (or x-y) numbering with even line and plane sizes");
    if (!(nrows >= (int64_t(1) << 20) || opt.sweep == 2)) return no_walk("below 2^20 rows (SCHWZ_SPMV_SWEEP=2 walks anyway)");
    if (nrows < 3 * PL || nrows % 2 || ncols != nrows) return no_walk("fewer than three planes, or not square");
    if (rle.empty()) return no_walk("chunks have no run-length records");
    const int nchunks = (int)((nrows + kPairRows - 1) / kPairRows);
    const int nplanes = (int)(nrows / PL), cpp = (int)(PL / kPairRows);
    // ---- per plane: the far offsets its rows use -------------------------------------------------
    auto in_plane = [&](schwz_idx off) { return off == 0 || off == 1 || off == -1 || off == NX || off == -NX; };
    std::vector<std::vector<schwz_idx>> pat_far((size_t)tb.npat);
    std::vector<uint8_t> pat_bad((size_t)tb.npat, 0);
    for (int q = 0; q < tb.npat; ++q) {
        if ((int)tb.len[(size_t)q] > 9) pat_bad[(size_t)q] = 1;
        for (int k = 0; k < (int)tb.len[(size_t)q]; ++k) {
            const schwz_idx off = tb.ent[(size_t)q * tb.lmax + k].off;
            if (in_plane(off)) continue;
            if (off % PL != 0) pat_bad[(size_t)q] = 1;  // a far entry must keep the in-plane position
            pat_far[(size_t)q].push_back(off);
        }
    }
    std::vector<uint8_t> plane_ok((size_t)nplanes, 1);
    std::vector<std::vector<schwz_idx>> plane_far((size_t)nplanes);  // sorted ascending
    std::vector<std::vector<int>> plane_pats((size_t)nplanes);
    for (int k = 0; k < nplanes; ++k) {
        std::vector<uint8_t> used((size_t)tb.npat, 0);
        if (gen_mode)  // the patterns of the plane's pairs, from the byte ids
            for (int64_t pr = (int64_t)k * PL / 2; pr < (int64_t)(k + 1) * PL / 2; ++pr) used[(size_t)P.pair_id[(size_t)pr]] = 1;
        for (int c = k * cpp; !gen_mode && c < (k + 1) * cpp && plane_ok[(size_t)k]; ++c) {
            const int R = P.rle_runs;
            if (rle[(size_t)c * R] == 0xffffu) {  // ids must run-length code (scalar loads only)
                plane_ok[(size_t)k] = 0;
                break;
            }
            // the patterns of a chunk are the ids of its runs
            for (int r = 0; r < R; ++r) used[(size_t)(rle[(size_t)c * R + r] >> 8)] = 1;
        }
        if (!plane_ok[(size_t)k]) continue;
        std::vector<schwz_idx> far;
        for (int q = 0; q < tb.npat; ++q) {
            if (!used[(size_t)q]) continue;
            plane_pats[(size_t)k].push_back(q);
            if (pat_bad[(size_t)q]) plane_ok[(size_t)k] = 0;
            for (schwz_idx f : pat_far[(size_t)q]) far.push_back(f);
        }
        std::sort(far.begin(), far.end());
        far.erase(std::unique(far.begin(), far.end()), far.end());
        int nb = 0, na = 0;
        for (schwz_idx f : far) {
            const int64_t j = k + f / PL;
            if (j < 0 || j >= nplanes) plane_ok[(size_t)k] = 0;
            (f < 0 ? nb : na)++;
        }
        if (far.size() > 2 || nb > 2 || na > 2) plane_ok[(size_t)k] = 0;
        if (plane_ok[(size_t)k]) plane_far[(size_t)k] = far;
    }
    // ---- chains: planes linked by their far couplings (degree <= 2: paths) ------------------------
    std::vector<std::vector<int>> adj((size_t)nplanes);
    auto link = [&](int x, int y) {
        if (std::find(adj[(size_t)x].begin(), adj[(size_t)x].end(), y) == adj[(size_t)x].end()) adj[(size_t)x].push_back(y);
    };
    for (int k = 0; k < nplanes; ++k)
        for (schwz_idx f : plane_far[(size_t)k]) {
            link(k, (int)(k + f / PL));
            link((int)(k + f / PL), k);
        }
    for (int k = 0; k < nplanes; ++k)
        if (adj[(size_t)k].size() > 2) {  // a plane somebody else points at as a third neighbour: not a path
            plane_ok[(size_t)k] = 0;
            for (int j : adj[(size_t)k]) plane_ok[(size_t)j] = 0;
        }
    std::vector<int> &chain_plane = W.chain_plane;  // concatenated chains, -1 between them and at both ends
    std::vector<int> pos_of((size_t)nplanes, -1);
    chain_plane.push_back(-1);
    std::vector<uint8_t> seen((size_t)nplanes, 0);
    for (int pass = 0; pass < 2; ++pass)   // paths from their ends first, then whatever is left (rings: cut anywhere)
        for (int k0 = 0; k0 < nplanes; ++k0) {
            if (seen[(size_t)k0] || adj[(size_t)k0].size() > 2) continue;
            if (pass == 0 && adj[(size_t)k0].size() != 1 && !adj[(size_t)k0].empty()) continue;
            int prev = -1, k = k0;
            while (k >= 0 && !seen[(size_t)k] && adj[(size_t)k].size() <= 2) {
                seen[(size_t)k] = 1;
                pos_of[(size_t)k] = (int)chain_plane.size();
                chain_plane.push_back(k);
                int next = -1;
                for (int j : adj[(size_t)k])
                    if (j != prev && !seen[(size_t)j]) next = j;
                prev = k;
                k = next;
            }
            chain_plane.push_back(-1);
        }
    const int npos = (int)chain_plane.size();
    for (int k = 0; k < 4; ++k) chain_plane.push_back(-1);  // the kernels look up to four positions ahead
    // ---- per chain position: which window each far slot reads; per pattern: its nine slots --------
    // far code: 2 bits per far slot (B0, B1, A0, A1): 0 none, 1 previous chain position, 2 next
    W.chain_far.assign((size_t)npos + 4, 0);
    std::vector<double> &cval = W.canon_val, &sval = W.canon_sym_val;
    std::vector<int> &cmsk = W.canon_mask, &smsk = W.canon_sym_mask;
    cval.assign((size_t)tb.npat * 18, 0.0);
    sval.assign((size_t)tb.npat * 10, 0.0);
    cmsk.assign((size_t)tb.npat, 0);
    smsk.assign((size_t)tb.npat, 0);
    std::vector<int8_t> pat_slot_set((size_t)tb.npat, 0);
    std::vector<std::vector<int8_t>> pat_slots((size_t)tb.npat);
    bool sym_ok = ts != nullptr && ts->npat == tb.npat;
    for (int p = 0; p < npos; ++p) {
        const int k = chain_plane[(size_t)p];
        if (k < 0 || !plane_ok[(size_t)k]) continue;
        const std::vector<schwz_idx> &far = plane_far[(size_t)k];
        std::vector<schwz_idx> fb, fa;
        for (schwz_idx f : far) (f < 0 ? fb : fa).push_back(f);
        int code = 0;
        bool ok = true;
        auto src_of = [&](schwz_idx f) -> int {
            const int j = (int)(k + f / PL);
            if (pos_of[(size_t)j] == p - 1) return 1;
            if (pos_of[(size_t)j] == p + 1) return 2;
            ok = false;
            return 0;
        };
        for (size_t i = 0; i < fb.size(); ++i) code |= src_of(fb[i]) << (2 * (int)i);
        for (size_t i = 0; i < fa.size(); ++i) code |= src_of(fa[i]) << (4 + 2 * (int)i);
        // slots of every pattern of the plane; a pattern shared with another plane must get the same ones
        for (int q : plane_pats[(size_t)k]) {
            std::vector<int8_t> slots;
            for (int e = 0; e < (int)tb.len[(size_t)q] && ok; ++e) {
                const schwz_idx off = tb.ent[(size_t)q * tb.lmax + e].off;
                int slot = -1;
                if (off == -NX) slot = 2;
                else if (off == -1) slot = 3;
                else if (off == 0) slot = 4;
                else if (off == 1) slot = 5;
                else if (off == NX) slot = 6;
                else {
                    for (size_t i = 0; i < fb.size(); ++i)
                        if (fb[i] == off) slot = (int)i;
                    for (size_t i = 0; i < fa.size(); ++i)
                        if (fa[i] == off) slot = 7 + (int)i;
                }
                if (slot < 0) ok = false;
                slots.push_back((int8_t)slot);
            }
            if (!ok) break;
            if (pat_slot_set[(size_t)q] && pat_slots[(size_t)q] != slots) ok = false;
            if (!ok) break;
            pat_slot_set[(size_t)q] = 1;
            pat_slots[(size_t)q] = slots;
        }
        if (!ok) {
            plane_ok[(size_t)k] = 0;
            continue;
        }
        W.chain_far[(size_t)p] = code;
    }
    for (int q = 0; q < tb.npat; ++q) {
        if (!pat_slot_set[(size_t)q]) continue;
        for (int e = 0; e < (int)tb.len[(size_t)q]; ++e) {
            const PairEntryH &en = tb.ent[(size_t)q * tb.lmax + e];
            const int slot = pat_slots[(size_t)q][(size_t)e];
            std::memcpy(&cval[((size_t)q * 9 + slot) * 2], &en.va, 8);
            std::memcpy(&cval[((size_t)q * 9 + slot) * 2 + 1], &en.vb, 8);
            cmsk[(size_t)q] |= (en.flags & 1) << slot;
            cmsk[(size_t)q] |= ((en.flags >> 1) & 1) << (16 + slot);
        }
        if (sym_ok) {
            // upper-triangle twin: slots [0, +1, +NX, far after 0, far after 1] = slots 4 .. 8 of the full form
            for (int e = 0; e < (int)ts->len[(size_t)q]; ++e) {
                const PairEntryH &en = ts->ent[(size_t)q * ts->lmax + e];
                int slot = -1;
                for (int f = 0; f < (int)tb.len[(size_t)q]; ++f)
                    if (tb.ent[(size_t)q * tb.lmax + f].off == en.off) slot = pat_slots[(size_t)q][(size_t)f] - 4;
                if (slot < 0 || slot > 4) {
                    sym_ok = false;
                    break;
                }
                std::memcpy(&sval[((size_t)q * 5 + slot) * 2], &en.va, 8);
                std::memcpy(&sval[((size_t)q * 5 + slot) * 2 + 1], &en.vb, 8);
                smsk[(size_t)q] |= (en.flags & 1) << slot;
                smsk[(size_t)q] |= ((en.flags >> 1) & 1) << (16 + slot);
            }
        }
    }
    if (!sym_ok) {
        sval.clear();
        smsk.clear();
    }
    // ---- segments -----------------------------------------------------------------------------------
    int T = opt.sweep_T ? *opt.sweep_T : ((NX >= 512 || (two_d && PL % 1024 == 0)) ? 1024 : 512);
    if (T != 512 && T != 1024) T = 512;
    if (PL % T && !gen_mode) T = 512;
    if (gen_mode && PL < T) T = 512;
    // Too many patterns for the tall band's LDS: the short one; still too much: no walk (the chunk-by-chunk
    // launches take the matrix).
    auto walk_lds = [&](int t) { return sweep_update_lds(t, NX, tb.npat); };
    if (walk_lds(T) > kSweepLdsLimit && T == 1024 && PL % 512 == 0) T = 512;
    if (walk_lds(T) > kSweepLdsLimit) return no_walk("ring and pattern tables exceed 96 KiB of LDS");
    if (NX > T) return no_walk("x line longer than a band");  // the halo of a band is NX rows either side: a band holds at least one x line
    const int bands = (int)((PL + T - 1) / T);
    std::vector<Run> runs;
    int64_t steps = 0;
    for (int p = 0; p < npos;) {
        const int k = chain_plane[(size_t)p];
        if (k < 0 || !plane_ok[(size_t)k]) {
            ++p;
            continue;
        }
        int e = p;
        while (e < npos && chain_plane[(size_t)e] >= 0 && plane_ok[(size_t)chain_plane[(size_t)e]]) ++e;
        if (e - p >= 2) {
            runs.push_back({p, e});
            steps += (int64_t)(e - p) * bands;
        }
        p = e;
    }
    if (runs.empty()) return no_walk("no chain of two or more walkable planes");
    std::vector<uint8_t> covered((size_t)nchunks, 0);
    std::vector<schwz_idx> &gen = W.gen;
    if (gen_mode) {
        // every plane must be walked: nothing can be left to the chunk-by-chunk companion launch
        int64_t walked = 0;
        for (const Run &r : runs) walked += r.p1 - r.p0;
        if (walked != nplanes) return no_walk("planes that are not whole chunks: some plane cannot be walked (and nothing can be left to the chunk launches)");
    } else {
        for (const Run &r : runs)
            for (int p = r.p0; p < r.p1; ++p)
                for (int c = 0; c < cpp; ++c) covered[(size_t)chain_plane[(size_t)p] * cpp + c] = 1;
        for (int c = 0; c < nchunks; ++c)
            if (!covered[(size_t)c]) gen.push_back(c);
    }
    // segment length: about three segments per CU (two for bands of 1024 rows, which keep twice the loads
    // in flight) in ONE round of workgroups (measured on MI355X, 256^3 and 512 x 512 x 64; tools/sweep_ab.sh)
    const int L = segment_length(runs, PL, T, opt.sweep_L, T == 1024 ? 2 : 3, cus, 8);
    // the companion launch walks its chunks with one gather round trip after the other: as many workgroups
    // as the partial-sum slots next to the segments allow (up to one per chunk)
    const int seg_slots = (int)((segment_count(runs, bands, L) + kXcds - 1) / kXcds * kXcds) + kXcds;
    const int gen_blocks = (int)std::min<int64_t>((int64_t)gen.size(), std::max(256, std::min(1024, grid - seg_slots)));
    W.seg = walk_segment_table(runs, PL, T, L, cus, opt.sweep_trim, 8, 4, grid - gen_blocks);
    // The fused direction launch may take taller bands than the update launch (SCHWZ_SWEEP_TDIR=512|1024|2048):
    // its window carries an NX-row halo of r AND p per band, so a band of twice the rows halves that share,
    // while the update launch keeps four halo lines per window and prefers the shorter band.  A table of its
    // own; equal to the update launch's when the band heights coincide.
    // Measured in-box (tools/tdir_ab.sh): 256-wide planes, update bands of 512 rows: 1024-row bands for the fused
    // launch -3 % per step (2048: +5 %); 512-wide planes, 1024 / 2048: +3 % (two workgroups per CU); 1024-wide
    // planes, where a 1024-row band is a single x line, 2048: fused launch 0.773 -> 0.696 ms, -4 % per step -- in
    // round 2.  With the halo three positions ahead (round 3) the halo lines hit L2 and what counts on 1024-wide
    // planes is the second workgroup per CU a 1024-row band leaves room for: 1024 x 1024 x 128 slab, fused launch
    // 0.681 ms with 2048-row bands, 0.640 ms with 1024 (step 16.5 -> 16.0 ms; profiles/r03_c5slab_ab.txt).
    int T_dir = opt.sweep_Tdir ? *opt.sweep_Tdir : (T == 512 ? 1024 : T);
    if ((T_dir != 512 && T_dir != 1024 && T_dir != 2048) || (PL % T_dir && !gen_mode) || (gen_mode && PL < T_dir) ||
        sweep_dirdot_lds(T_dir, NX, tb.npat, dirdot_halo_lines) > kSweepLdsLimit)
        T_dir = T;
    if (T_dir != T) {
        const int Ld = segment_length(runs, PL, T_dir, opt.sweep_Ldir, T_dir >= 2048 ? 1 : (T_dir == 1024 ? 2 : 3), cus, 8);
        W.seg_dir = walk_segment_table(runs, PL, T_dir, Ld, cus, opt.sweep_trim_dir, 8, 4, grid - gen_blocks);
        if ((int64_t)W.seg_dir.size() + gen_blocks > grid) W.seg_dir.clear();
    }
    if (W.seg_dir.empty()) T_dir = T;
    // Rows the walk leaves out cost a companion launch per CG launch: measured with 256 x 256 planes, 8 / 4 / 1
    // slabs on one GPU when the boundary planes of a slab were still left out (tools/sweep_sizes.sh, bench.py
    // --ttr-subdomains): +13 % time at 2.2 M rows, +2 % at 4.3 M, -18 % at 16.8 M; without left-out rows the
    // walk wins from 1 M rows on.
    const bool worth = gen.empty() || nrows >= 6000000 || opt.sweep == 2;
    if (!worth || (int64_t)W.seg.size() + gen_blocks > grid || steps * T * 2 < nrows)
        return no_walk("rows left to the companion launch on a small matrix, more segments than partial-sum slots, or less than half of the rows walkable");
    // A table of its own for the first-direction launch of a solve (round 3).  That launch reads ONE vector and does
    // little per row: its time is the latency of a workgroup's steps times the bytes it keeps in flight, and the
    // fused launch's table gives it two workgroups per CU.  Bands of the update launch's height (512 rows where the
    // plane allows; a height both walks have instantiations for) and about SCHWZ_SWEEP_FIRSTPERCU (6; 0: the fused
    // launch's table) workgroups per CU.
    W.T_first = T_dir;
    if (opt.sweep_first_per_cu > 0 && T <= T_dir) {
        const int Lf = segment_length(runs, PL, T, std::nullopt, opt.sweep_first_per_cu, cus, 6);
        W.seg_first = walk_segment_table(runs, PL, T, Lf, cus, opt.sweep_trim_first, 6, 2, grid - gen_blocks);
        if ((int64_t)W.seg_first.size() + gen_blocks > grid) W.seg_first.clear();
        else W.T_first = T;
    }
    // ---- what the kernels read at entry: a record per slot, the tables ready to stage (coding_plan.hpp) ----
    auto records = [&](const std::vector<int4> &seg) {
        std::vector<WalkRecord> out(seg.size());
        for (size_t i = 0; i < seg.size(); ++i) {
            WalkRecord &r = out[i];
            r.band = seg[i].x;
            r.z0 = seg[i].y;
            r.z1 = seg[i].z;
            r.rows = seg[i].w;
            for (int k = 0; k < 5; ++k) {
                const int64_t p = (int64_t)r.z0 - 1 + k;
                r.plane[k] = p >= 0 && p < (int64_t)chain_plane.size() ? chain_plane[(size_t)p] : -1;
            }
            r.pad[0] = r.pad[1] = r.pad[2] = 0;
        }
        return out;
    };
    W.rec = records(W.seg);
    W.rec_dir = records(W.seg_dir);
    W.rec_first = records(W.seg_first);
    auto ready = [](const std::vector<double> &val, const std::vector<int> &mask, int slots) {
        std::vector<double> out(val.size(), 0.0);
        for (size_t q = 0; q < mask.size(); ++q)
            for (int k = 0; k < slots; ++k)
                for (int b = 0; b < 2; ++b)
                    if ((mask[q] >> (16 * b + k)) & 1) out[(q * slots + k) * 2 + b] = val[(q * slots + k) * 2 + b];
        return out;
    };
    W.canon_ready = ready(cval, cmsk, 9);
    W.canon_sym_ready = ready(sval, smsk, 5);
    W.gen_mode = gen_mode ? 1 : 0;
    W.T = T;
    W.T_dir = T_dir;
    W.nx = (int)NX;
    W.pl = PL;
    W.npat = tb.npat;
    W.gen_blocks = gen_blocks;
    return W;
}

DualPlan plan_dual_split(int64_t nrows, const schwz_idx *rp, const schwz_idx *col, int64_t split,
                         const std::vector<int> &chain_plane, int64_t walk_pl)
{
    DualPlan D;
    const int nchunks = (int)((nrows + kPairRows - 1) / kPairRows);
    D.chunk_dual.assign((size_t)nchunks, 0);
    for (int c = 0; c < nchunks; ++c) {
        const int64_t r0 = (int64_t)c * kPairRows, r1 = std::min<int64_t>(r0 + kPairRows, nrows);
        bool f = r1 > split;
        for (int64_t j = rp[r0]; j < rp[r1] && !f; ++j) f = col[j] >= split;
        D.chunk_dual[(size_t)c] = f ? 1 : 0;
    }
    if (walk_pl <= 0) return D;
    // the same for the z-sweep walk: chain positions whose plane has a flagged chunk, and the list of those
    // planes' chunks for the listed kSpmvResidNorm launch (launch_spmv_pair, dual start in the walk)
    const int cpp = (int)(walk_pl / kPairRows);
    D.chain_dual.assign(chain_plane.size(), 0);
    for (size_t p = 0; p < chain_plane.size(); ++p) {
        const int k = chain_plane[p];
        if (k < 0) continue;
        bool f = false;
        for (int c = k * cpp; c < (k + 1) * cpp && c < nchunks; ++c) f = f || D.chunk_dual[(size_t)c];
        if (!f) continue;
        D.chain_dual[p] = 1;
        for (int c = k * cpp; c < (k + 1) * cpp && c < nchunks; ++c) D.dual_chunks.push_back(c);
    }
    if (D.dual_chunks.empty()) D.chain_dual.clear();
    D.dual_blocks = (int)std::min<size_t>(D.dual_chunks.size(), 512);
    return D;
}

}  // namespace schwz
