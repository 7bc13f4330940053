// Internal declarations shared by the translation units of libschwz_hip.so.
// Not part of the ABI (include/schwz_hip.h is).
#pragma once

#include <hip/hip_runtime_api.h>

#include <sched.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <string>
#include <sys/mman.h>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "schwz_hip.h"

namespace schwz {

// std::allocator whose construct() default-initialises: resize() of a vector of arithmetic type leaves the new
// elements unwritten instead of zero-filling them on one thread.
template <typename T>
struct NoInitAlloc : std::allocator<T> {
    template <typename U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <typename U>
    NoInitAlloc(const NoInitAlloc<U> &) {}
    template <typename U>
    void construct(U *p) { ::new ((void *)p) U; }
    template <typename U, typename... Args>
    void construct(U *p, Args &&...args) { ::new ((void *)p) U(std::forward<Args>(args)...); }
    // Large blocks (the local matrix: 1.4 GB at 256^3) come 2 MiB-aligned and marked for transparent huge pages:
    // their first touch is then one fault per 2 MiB instead of 512 -- on a kernel in `madvise` mode the setup's
    // page faults were a third of its time (SCHWZ_SETUP_HUGEPAGES=0: plain operator new).
    static bool huge_pages()
    {
        static const bool v = [] {
            const char *e = std::getenv("SCHWZ_SETUP_HUGEPAGES");
            return !(e && e[0] == '0');
        }();
        return v;
    }
    static constexpr size_t kHugeMin = size_t(8) << 20, kHugeAlign = size_t(2) << 20;
    T *allocate(size_t n)
    {
        const size_t bytes = n * sizeof(T);
        if (bytes >= kHugeMin && huge_pages()) {
            void *p = nullptr;
            const size_t padded = (bytes + kHugeAlign - 1) / kHugeAlign * kHugeAlign;
            if (posix_memalign(&p, kHugeAlign, padded) == 0) {
                (void)madvise(p, padded, MADV_HUGEPAGE);
                return static_cast<T *>(p);
            }
            p = std::malloc(bytes);  // (deallocate() frees blocks of this size with std::free)
            if (!p) throw std::bad_alloc();
            return static_cast<T *>(p);
        }
        return static_cast<T *>(::operator new(bytes));
    }
    void deallocate(T *p, size_t n)
    {
        if (n * sizeof(T) >= kHugeMin && huge_pages())
            std::free(p);
        else
            ::operator delete(p);
    }
};

// Threads for the host-side setup loops: SCHWZ_SETUP_THREADS, else the smallest of the CPUs this process may run on,
// its cgroup CPU quota (a GPU box shows all 256 hardware threads of the host to a job that may use 16 of them:
// an OpenMP team of 256 on that quota made every setup stage 2-5 x slower and erratic) and 32 -- divided by the
// ranks of this node when a launcher says how many there are.
inline int setup_threads()
{
    static const int v = [] {
        const char *e = std::getenv("SCHWZ_SETUP_THREADS");
        int n = e ? std::atoi(e) : 0;
        if (n > 0) return n > 256 ? 256 : n;
        cpu_set_t set;
        n = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
        auto quota = [](const char *path_quota, const char *path_period) -> double {
            // cgroup v2: "cpu.max" holds "<quota|max> <period>"; v1: two files
            double q = -1.0, per = -1.0;
            if (FILE *f = std::fopen(path_quota, "r")) {
                char word[64] = {0};
                if (path_period == nullptr) {
                    if (std::fscanf(f, "%63s %lf", word, &per) == 2 && word[0] != 'm') q = std::atof(word);
                } else if (std::fscanf(f, "%lf", &q) != 1) {
                    q = -1.0;
                }
                std::fclose(f);
            }
            if (path_period)
                if (FILE *f = std::fopen(path_period, "r")) {
                    if (std::fscanf(f, "%lf", &per) != 1) per = -1.0;
                    std::fclose(f);
                }
            return q > 0.0 && per > 0.0 ? q / per : -1.0;
        };
        double cpus = quota("/sys/fs/cgroup/cpu.max", nullptr);
        if (cpus <= 0.0) cpus = quota("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "/sys/fs/cgroup/cpu/cpu.cfs_period_us");
        if (cpus > 0.0) n = std::min(n, (int)(cpus + 0.999));
        // one rank per GPU of a node (torch.distributed.run / mpiexec set these): the ranks share those CPUs
        for (const char *var : {"LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_LOCAL_SIZE", "MPI_LOCALNRANKS"}) {
            const char *w = std::getenv(var);
            const int ranks = w ? std::atoi(w) : 0;
            if (ranks > 1) {
                n = std::max(1, n / ranks);
                break;
            }
        }
        return n < 1 ? 1 : (n > 32 ? 32 : n);
    }();
    return v;
}

// Host-side setup loops of the .hip translation units (hipcc builds them without an OpenMP runtime): fn(t, nt,
// begin, end) on nt threads over contiguous blocks of [0, n), thread t taking the t-th block.  nt = setup_threads(),
// 1 below min_per_thread items per thread.  Returns nt.
template <typename F>
inline int parallel_blocks(int64_t n, int64_t min_per_thread, F fn)
{
    const int cap = setup_threads();
    int nt = (int)std::min<int64_t>(cap, n / std::max<int64_t>(min_per_thread, 1));
    if (nt < 1) nt = 1;
    if (nt == 1) {
        fn(0, 1, (int64_t)0, n);
        return 1;
    }
    std::vector<std::thread> th;
    th.reserve((size_t)nt - 1);
    for (int t = 1; t < nt; ++t) th.emplace_back([=, &fn] { fn(t, nt, n * t / nt, n * (t + 1) / nt); });
    fn(0, nt, (int64_t)0, n / nt);
    for (auto &x : th) x.join();
    return nt;
}

// SCHWZ_SETUP_TIMING=1: wall time of the setup stages on stderr ("[schwz setup] <stage>: <ms> ms"), what
// tools/setup_probe.py reads.  Zero cost when off.
struct StageTimer {
    const char *name;
    std::chrono::steady_clock::time_point t0;
    bool on;
    explicit StageTimer(const char *n) : name(n), on(false)
    {
        static const bool enabled = [] {
            const char *e = std::getenv("SCHWZ_SETUP_TIMING");
            return e && e[0] == '1';
        }();
        on = enabled;
        if (on) t0 = std::chrono::steady_clock::now();
    }
    void stop()
    {
        if (!on) return;
        on = false;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::fprintf(stderr, "[schwz setup] %s: %.1f ms\n", name, ms);
    }
    ~StageTimer() { stop(); }
};

void set_error(const std::string &msg);

#define SCHWZ_HIP_TRY(expr)                                                        \
    do {                                                                           \
        hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess) {                                                    \
            ::schwz::set_error(std::string(__FILE__) + ":" + std::to_string(__LINE__) + \
                               ": " #expr " -> " + hipGetErrorString(e_));         \
            return SCHWZ_ERR_HIP;                                                  \
        }                                                                          \
    } while (0)

#define SCHWZ_REQUIRE(cond, msg)                      \
    do {                                              \
        if (!(cond)) {                                \
            ::schwz::set_error(std::string(msg));     \
            return SCHWZ_ERR_INVALID;                 \
        }                                             \
    } while (0)

// A device allocation that frees itself.  The buffers of the matrix codings live in structs of these
// (schwz_csr::coding): releasing a coding is assigning a fresh struct, and no pointer can be forgotten.
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        std::swap(p, o.p);
        return *this;
    }
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    // replaces the allocation by `bytes` fresh ones (at least 16), zeroed on request
    int alloc(size_t bytes, bool zero = false)
    {
        *this = DevBuf();
        bytes = bytes ? bytes : 16;
        SCHWZ_HIP_TRY(hipMalloc(&p, bytes));
        if (zero) SCHWZ_HIP_TRY(hipMemset(p, 0, bytes));
        return SCHWZ_OK;
    }
    // replaces the allocation by a copy of h[0:count]; `pad` extra zeroed elements follow the data (the 16-byte
    // SpMV loads may touch them)
    template <typename T>
    int put(const T *h, size_t count, size_t pad = 0)
    {
        *this = DevBuf();
        SCHWZ_HIP_TRY(hipMalloc(&p, (count + pad ? count + pad : 1) * sizeof(T)));
        if (count) SCHWZ_HIP_TRY(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
        if (pad) SCHWZ_HIP_TRY(hipMemset((char *)p + count * sizeof(T), 0, pad * sizeof(T)));
        return SCHWZ_OK;
    }
    template <typename T, typename A>
    int put(const std::vector<T, A> &h, size_t pad = 0)
    {
        return put(h.data(), h.size(), pad);
    }
    // hands the allocation to the caller, who frees it (the C ABI's out pointers: schwz_device_free)
    void *release()
    {
        void *q = p;
        p = nullptr;
        return q;
    }
    template <typename T>
    const T *as() const { return static_cast<const T *>(p); }
};

// ... of `count` T, handed to launches as the T * it converts to.  The vectors and scalars of the solver objects
// are these: destroying a solver is `delete`, and a create that fails half way leaves nothing behind.
template <typename T>
struct Dev : DevBuf {
    int alloc(size_t count, bool zero = false) { return DevBuf::alloc(count * sizeof(T), zero); }
    // (of T only: these hide DevBuf's put of any element type)
    int put(const T *h, size_t count, size_t pad = 0) { return DevBuf::put(h, count, pad); }
    template <typename A>
    int put(const std::vector<T, A> &h, size_t pad = 0) { return DevBuf::put(h.data(), h.size(), pad); }
    operator T *() const { return static_cast<T *>(p); }
};

// pinned host memory that frees itself
template <typename T>
struct Pinned {
    T *p = nullptr;
    Pinned() = default;
    Pinned(const Pinned &) = delete;
    ~Pinned()
    {
        if (p) (void)hipHostFree(p);
    }
    int alloc(size_t count, unsigned flags = hipHostMallocDefault)  // zeroed
    {
        SCHWZ_HIP_TRY(hipHostMalloc((void **)&p, count * sizeof(T), flags));
        std::memset(p, 0, count * sizeof(T));
        return SCHWZ_OK;
    }
};

// a HIP handle that destroys itself and converts to the raw handle the runtime calls take
template <typename H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    explicit Handle(H h_) : h(h_) {}
    Handle(Handle &&o) noexcept : h(o.h) { o.h = nullptr; }
    Handle &operator=(Handle &&o) noexcept
    {
        std::swap(h, o.h);
        return *this;
    }
    ~Handle()
    {
        if (h) (void)Destroy(h);
    }
    operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    int create()  // (no timing: an ordering point only)
    {
        SCHWZ_HIP_TRY(hipEventCreateWithFlags(&h, hipEventDisableTiming));
        return SCHWZ_OK;
    }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    int create()  // non-blocking
    {
        SCHWZ_HIP_TRY(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
        return SCHWZ_OK;
    }
};
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;
using Graph = Handle<hipGraph_t, hipGraphDestroy>;  // the temporary of a stream capture

}  // namespace schwz

#include "solver_state.hpp"

namespace schwz {

// ---- SpMV tiling constants (see DESIGN.md "CSR SpMV") ------------------------
constexpr int kBlock = 256;      // threads per workgroup = 4 waves of 64
constexpr int kTileNnz = 2048;   // products staged in LDS per tile (16 KiB fp64)
constexpr int kTileRows = 256;   // one lane per row in the reduction phase
constexpr int kMaxGrid = 2048;   // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int kXcds = 8;

// What a z-sweep walk workgroup needs to know before it can request its first windows, in one record per workgroup
// slot (plan_walk, coding_plan.cpp): the slot's entry of the segment table {band, z0, z1, rows of the band} and the
// plane indices of the chain positions z0 - 1 .. z0 + 3 (-1: no plane there), which the kernels would otherwise look
// up in chain_plane behind the segment.  48 bytes: two scalar loads.
struct alignas(16) WalkRecord {
    int band, z0, z1, rows;
    int plane[5];
    int pad[3];
};
static_assert(sizeof(WalkRecord) == 48, "a walk record is three 16-byte pieces");

constexpr int kGraphIters = 16;         // CG iterations per recorded hipGraph (even: rho slots repeat)
constexpr int64_t kGraphRows = 1 << 21;  // systems up to this many rows replay their CG loop as graphs
constexpr int kDeferDepth = 16;          // search directions kept before x += sum alpha_k p_k is applied
constexpr int kWaveTileNnz = 512;  // products staged per wave (4 KiB fp64)

struct CsrView {
    int64_t nrows = 0, ncols = 0, nnz = 0;
    const schwz_idx *rp = nullptr;
    const schwz_idx *col = nullptr;
    const double *val = nullptr;
    int ntiles = 0;
    const schwz_idx *tile_row = nullptr;  // ntiles+1 row boundaries
    const schwz_idx *tile_order = nullptr;  // optional BFS visiting order (SCHWZ_TILE_ORDER=1)
    // spmv_stream.hip: first nonzero of every tile (rp[tile_row[t]], ntiles+1 entries) and the masked-add count
    // of its row sums (8 / 16 / 32 >= the longest row; 0: the matrix keeps spmv_tiled2_kernel)
    const schwz_idx *tile_nz = nullptr;
    int stream_cap = 0;
    // spmv_stream.hip: slots per bank of the scratch (SpmvArgs::stream_part) a launch needs whose grid exceeds the
    // kMaxGrid slots the consumers fold; 0: no launch on this matrix does.  The scratch belongs to whoever launches
    int stream_part_cap = 0;
    // spmv_stream.hip on wide planes: the tile sequence of every XCD, laid out explicitly (entry [xcd * stream_nper + j],
    // -1 past the end) so that a tile's +-plane neighbours are close in the sequence; null: the block-cyclic deal
    const schwz_idx *stream_order = nullptr;
    int stream_nper = 0;
    int xcd_block = 0;  // tiles are dealt to the 8 XCDs block-cyclically in runs of this many (a power of two)
    int xcd_shift = 0;  // log2(xcd_block)
    // kSpmvResidDual: 1 where the tile's rows or columns reach past `dual_split` (where x2 may
    // differ from x); elsewhere the second product is skipped (nullptr: every tile)
    const uint8_t *tile_dual = nullptr;
    int nwtiles = 0;                        // wave tiles: <= 64 rows, <= kWaveTileNnz-2 nnz
    const schwz_idx *wtile_row = nullptr;
    // dictionary-coded copy of (val, col) for the tiles that allow it (spmv_dict.hip):
    // code[j] = value code | delta code << 8 ; per tile a value and a (col - row) dictionary
    const uint16_t *code = nullptr;
    const schwz_idx *vdict_ptr = nullptr;   // ntiles+1 ; vdict_ptr[t] == vdict_ptr[t+1] => raw tile
    const schwz_idx *ddict_ptr = nullptr;   // ntiles+1
    const double *vdict = nullptr;
    const schwz_idx *ddict = nullptr;
    // row-pattern coding (spmv_dict.hip): one byte per row selects a (values, col - row offsets)
    // pattern from a small table shared by many tiles
    const uint8_t *pat_id = nullptr;        // nrows
    const schwz_idx *tile_table = nullptr;  // ntiles: table id, -1 = tile not pattern coded
    const schwz_idx *tbl_desc = nullptr;    // per table: {entry offset, len offset, npat, lmax}
    const uint8_t *tbl_len = nullptr;       // pattern lengths, concatenated
    const double *tbl_val = nullptr;        // [npat][lmax] per table, concatenated
    const schwz_idx *tbl_delta = nullptr;
    // row-pair pattern coding (spmv_pair.hip): one byte per PAIR of adjacent rows selects a merged
    // (col - row, value of row r, value of row r+1, presence bits) sequence
    const uint8_t *pair_id = nullptr;        // (nrows + 1) / 2: pattern of rows (2i, 2i + 1)
    // the same ids run-length coded per chunk: 8 x (first pair of the run | id << 8), 16 bytes a chunk
    // read with one wave-uniform load instead of one byte per lane; first word 0xffff: more than 8
    // runs, the chunk's ids come from pair_id (nullptr: not built)
    const uint4 *pair_rle = nullptr;
    int sweep_gen_mode = 0;  // z-sweep walk over planes that are not whole 512-row chunks: byte ids, partial last band
    int pair_rle_runs = 8;  // runs per chunk record: 8 (16 bytes) or 16 (32 bytes, x lines shorter than ~170 entries)
    const schwz_idx *chunk_ptable = nullptr; // per chunk of 512 rows: pair table id, -1 = not pair coded
    const uint8_t *chunk_dual = nullptr;     // per chunk: the fused dual residual needs its second product
    int pair_shift = 0;                      // log2 of the run length of the XCD deal of the chunks
    int pair_single = 0;                     // 1: every chunk uses table 0
    const schwz_idx *ptbl_desc = nullptr;    // per table: {entry offset, len offset, npat, lmax, max |col - row|}
    const uint8_t *ptbl_len = nullptr;
    const double *ptbl_val = nullptr;        // 2 per entry
    const schwz_idx *ptbl_meta = nullptr;    // 2 per entry: offset, flags
    // symmetric matrices only: for table t, table pair_sym_base + t holds the entries with col >= row,
    // the strictly upper ones doubled: x.(A x) = sum_i x_i (a_ii x_i + 2 sum_{j>i} a_ij x_j) with about
    // half the gathers (kSpmvDotSym); 0 = not built
    int pair_sym_base = 0;
    // single-table matrices whose commonest pattern is a stencil row pair {n2, n1, -1, 0, +1, p1, p2}:
    // that offset layout (pair_canon[0..6]; pair_canon[7] != 0: valid).  Waves whose lanes all have
    // patterns inside the layout gather its 6 outer slots and take the operands of the offset-0 slot
    // from the -1 and +1 gathers.
    int pair_canon[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // z-sweep ("brick") walk of a canonical 3-D stencil layout {-PL, -NX, -1, 0, +1, +NX, +PL} (spmv_pair.hip):
    // a workgroup keeps a band of sweep_T rows and walks it through consecutive planes (stride PL), the
    // window [band - NX, band + T + NX) of each plane staged once in an LDS ring.  sweep_rec: one WalkRecord per
    // workgroup slot -- the segment {band, z0, z1, rows of the band} (z0 == z1: empty) and the planes of its first
    // five chain positions; sweep_gen: the chunks of 512 rows no segment covers (boundary planes of a subdomain,
    // overlap rows), walked the generic way by sweep_gen_blocks more workgroups of the same launch.
    // sweep_nslots == 0: not built.
    // (unused_*: seven tables the walks read in earlier forms -- segments as int4, slot values and presence masks.
    // Nothing uploads or reads them; the pointers keep their places, and stay null, because the argument block of
    // every kernel that takes a CsrView is laid out by this struct: without them the compiler schedules some of those
    // kernels differently (spmv_dict.hip: other VGPR counts, profiles/r25_walk_forms.txt).)
    int sweep_T = 0, sweep_nx = 0, sweep_nslots = 0, sweep_ngen = 0, sweep_gen_blocks = 0;
    int64_t sweep_pl = 0;
    const void *unused_seg = nullptr;
    // the fused direction launch's own band height and records (spmv_pair_dirdot_sweep_kernel); equal to the update
    // launch's unless SCHWZ_SWEEP_TDIR asks for taller bands
    int sweep_T_dir = 0, sweep_nslots_dir = 0;
    const void *unused_seg_dir = nullptr;
    // ... and the first-direction launch of a solve (one vector read, bound by latency: more, shorter workgroups)
    int sweep_T_first = 0, sweep_nslots_first = 0;
    const void *unused_seg_first = nullptr;
    const WalkRecord *sweep_rec = nullptr, *sweep_rec_dir = nullptr, *sweep_rec_first = nullptr;
    const schwz_idx *sweep_gen = nullptr;
    const void *unused_canon_val = nullptr, *unused_canon_mask = nullptr;
    int canon_npat = 0;  // patterns of table 0
    const void *unused_canon_sym_val = nullptr, *unused_canon_sym_mask = nullptr;
    // per pattern of table 0: its entries in the nine slots [far before 0, far before 1, -NX, -1, 0, +1, +NX,
    // far after 0, far after 1] as 9 pairs (row r, row r + 1), +0.0 where the pattern has no entry: the form the
    // walks keep in LDS (they sum every slot, spmv_pair.hip) -- one 16-byte load per staged entry
    const double *canon_ready = nullptr;
    // the same for the upper-triangle twin of the table (symmetric matrices; nullptr: none): slots [0, +1, +NX,
    // far after 0, far after 1], 5 pairs
    const double *canon_sym_ready = nullptr;
    // chains of planes (see plan_walk, coding_plan.cpp): plane index per chain position (-1: none) and, per position, which
    // window each far slot reads (2 bits per slot B0, B1, A0, A1: 0 none, 1 previous position, 2 next)
    const int *chain_plane = nullptr;
    const int *chain_far = nullptr;
    // fused dual residual in the walk (pair_set_dual_split): 1 per chain position whose plane holds or couples
    // to rows / columns >= the split (there b - A x2 may differ from b - A x); the chunks of those planes,
    // walked chunk by chunk by a second small launch (kSpmvResidNorm, listed) -- nullptr / 0: not built
    const int *chain_dual = nullptr;
    const schwz_idx *dual_chunks = nullptr;
    int dual_nchunks = 0, dual_blocks = 0;
};

// sequence slots per XCD of the block-cyclic deal of the tiles (runs of xcd_block tiles, whole runs per XCD)
__host__ __device__ inline int xcd_slots(const CsrView &A)
{
    const int sh = A.xcd_shift;
    return ((A.ntiles + (kXcds << sh) - 1) >> (sh + 3)) << sh;
}

// The tile pipeline over plain CSR (stream_pipeline.hpp): whether it takes the matrix, the slots of an XCD's sequence
// (the explicit one of wide planes, or the block-cyclic deal), and the instantiation for the matrix's longest row.
inline bool stream_takes(const CsrView &A) { return A.stream_cap != 0 && A.tile_nz && !A.tile_order; }

__host__ __device__ inline int stream_slots(const CsrView &A) { return A.stream_order ? A.stream_nper : xcd_slots(A); }

// f(std::integral_constant<int, CAP>) with CAP = 8 / 16 / 32, the smallest that holds A.stream_cap
template <typename F>
inline void stream_cap_dispatch(const CsrView &A, F &&f)
{
    if (A.stream_cap <= 8)
        f(std::integral_constant<int, 8>());
    else if (A.stream_cap <= 16)
        f(std::integral_constant<int, 16>());
    else
        f(std::integral_constant<int, 32>());
}

// epilogues of the tiled SpMV kernel
enum SpmvMode {
    kSpmvPlain = 0,      // y = alpha*A*x + beta*y
    kSpmvDot = 1,        // y = A*x ; partial[b] = sum x_i*y_i
    kSpmvResidInit = 2,  // r = b - A*x ; p = dinv*r ; partials sum r*z, sum r*r
    kSpmvResidNorm = 3,  // partial sum (b - A*x)^2, nothing stored
    // kSpmvResidInit on x plus, in the same pass over the matrix, the partial sum
    // (b - A*x2)^2 over rows < row_limit (third partial bank): the convergence-check
    // residual (solve.cpp:834-841) and the CG start residual share one matrix read
    kSpmvResidDual = 4,
    // row-pair kernel only (spmv_pair.hip): the CG iteration without a stored q = A p.
    kSpmvDotOnly = 5,    // partial sum x_i*(A x)_i, nothing stored
    // alpha = rho / fold(p.q partials); per row q_i = (A p)_i recomputed, x_i += alpha p_i,
    // r_i -= alpha q_i, partials r.z and r.r (what cg_update_kernel does, minus 16 B/row of q)
    kSpmvCgUpdate = 6,
    // kSpmvDotOnly for a matrix whose upload found it symmetric: the same number from the upper
    // triangle alone (CsrView::pair_sym_base), about half the gathers
    kSpmvDotSym = 7,
    // the direction update and the next iteration's kSpmvDotSym in one launch: beta from the folded
    // partials, p' = z + beta p computed wherever the upper-triangle gathers need it (own entry and
    // neighbours alike, from r and the OLD p, which this launch only reads), own p' stored to a
    // second buffer, partial sums of p'.(A p'); CgState advanced by workgroup 0
    kSpmvDirDotSym = 8,
    kSpmvDirDotSymVec = 9  // ... with the Jacobi diagonal as a full vector (gathered like r and p)
};

struct SpmvArgs {
    double alpha = 1.0, beta = 0.0;
    const double *x = nullptr;
    const double *x2 = nullptr;  // kSpmvResidDual: second vector (nullptr: same as x)
    double *y = nullptr;        // out vector (y / q / r)
    const double *b = nullptr;  // rhs for the residual modes
    double *p = nullptr;        // kSpmvResidInit: search direction out
    const double *dinv = nullptr;
    double *partials = nullptr;  // [2][grid] ([3][grid] for kSpmvResidDual)
    const int *stop_iter = nullptr;  // device flag checked by CG launches
    int it = 0;
    int64_t row_limit = 0;  // rows >= row_limit are skipped in kSpmvResidNorm
    // kSpmvCgUpdate
    double *cg_x = nullptr, *cg_r = nullptr;
    const struct CgState *cg_state = nullptr;
    const double *pq_partials = nullptr;
    int pq_nparts = 0;
    int diag_mode = 0;          // 0 none, 1 full vector (dinv), 3 uniform scalar
    double diag_uniform = 1.0;
    double cg_rtol = 0.0;       // kSpmvDirDotSym: relative tolerance of the stopping test
    // kSpmvCgUpdate with cg_x == nullptr: x is not touched, alpha is stored here instead (workgroup 0)
    double *alpha_out = nullptr;
    // set by launch_spmv_pair for the companion launch of the z-sweep walk: walk the chunks listed in
    // CsrView::sweep_gen only (2: CsrView::dual_chunks, kSpmvResidNorm); partial sums at
    // [part_offset + blockIdx.x] of banks part_stride apart
    int sweep = 0;
    int part_offset = 0, part_stride = 0;
    // kSpmvResidInit in the z-sweep walk (r stored, p left to the first direction launch), and that first
    // direction launch (kSpmvDirDotSym: p' = D^-1 r, CgState untouched); pcg_begin / pcg_iterate set them
    // where pair_sweep_start_ok holds
    int sweep_init = 0, sweep_first = 0;
    // spmv_stream.hip: consecutive tiles per workgroup of a grid that covers the matrix once (0: persistent
    // workgroups striding through their XCD's sequence, the form of round 2)
    int seq = 0;
    // spmv_stream.hip: scratch for the per-workgroup partial sums of such a launch, 2 banks of CsrView::stream_part_cap
    // doubles (stream_part_alloc).  It belongs to the object that launches -- a solver, a subdomain -- not to the
    // matrix, so that objects sharing a matrix can run on different streams; nullptr: the persistent form
    double *stream_part = nullptr;
    // q-free CG on the walks, a solve that started in the walk (round 3, "virtual first direction"): p0 = D^-1 r0 is
    // never stored -- the first update walk builds its windows from r0 (a.x = r0, windows x ring_scale) and writes
    // r1 to cg_r_out, so r0 stays intact for the first fused direction launch (a.x = r0, p read as p_scale x a.x)
    // and for the x update (slot 0 of the ring = r0 x the same factor).  p0_virtual = 1 marks such a launch: it must
    // be served by the walk kernels (launch_spmv_pair fails loudly otherwise).
    int p0_virtual = 0;
    double ring_scale = 1.0;
    double *cg_r_out = nullptr;
    double p_scale = 1.0;
    // kSpmvCgUpdate / kSpmvDirDotSym: whoever planned the launch wants the z-sweep walk (cg.hip's plan, from
    // pair_sweep_update_ok / pair_sweep_dirdot_ok); launch_spmv_pair reads no switch of its own
    int walk = 0;
    // first-direction launch of a solve that started in the walk (sweep_first): workgroup 0 also folds the start
    // launch's partial sums -- pq_partials, pq_nparts slots per bank; banks 0 and 1: rho and ||r||^2 -- into
    // cg_state with the stopping test of cg_rtol, and bank norm_bank into norm_sq_out (nullptr: no check norm):
    // what cg_init_finalize_kernel does (cg.hip, CgPlan::initfold)
    int init_fold = 0;
    int norm_bank = 1;
    double *norm_sq_out = nullptr;
    // launch timeline of the z-sweep walks (measurement builds of spmv_pair.hip only, -DSCHWZ_WITH_PROBES; the product
    // never sets or reads it): kWalkStampWords 64-bit words per workgroup of this launch, tools/walk_timeline.py
    unsigned long long *walk_probe = nullptr;
};

// SpmvArgs::stream_part for launches on A: empty where A needs none, or where the allocation fails (those launches
// keep the persistent form).  The solver or subdomain that launches moves it in
inline Dev<double> stream_part_alloc(const CsrView &A)
{
    Dev<double> part;
    if (A.stream_part_cap > 0 && part.alloc((size_t)2 * A.stream_part_cap)) (void)hipGetLastError();
    return part;
}

// launch grid of the streaming vector kernels: one lane per element up to kMaxGrid workgroups
inline int grid_for(int64_t n)
{
    int64_t g = (n + kBlock - 1) / kBlock;
    if (g > kMaxGrid) g = kMaxGrid;
    return g < 1 ? 1 : (int)g;
}

// small launch helpers shared by the translation units (defined in kernels.hip)
int launch_interface_update(int64_t nrows, int64_t row0, const schwz_idx *rp, const schwz_idx *col,
                            const double *val, const double *x, const double *b, double *bt, hipStream_t s);
int launch_final_norm(const double *partials, int nparts, double *out, hipStream_t s);
int launch_copy(int64_t n, const double *src, double *dst, hipStream_t s);
int launch_copy_any(int64_t n, const double *src, double *dst, hipStream_t s);  // outer.hip: any 8-byte alignment
int launch_gather_f32(int64_t n, const schwz_idx *idx, const double *from, float *into, hipStream_t s);
int launch_scatter_f32(int64_t n, const schwz_idx *idx, const float *from, double *into, hipStream_t s);

int spmv_grid(const CsrView &A, int variant);
// the SpMV variants whose kernels have the fused check + start residual mode (kSpmvResidDual)
inline bool spmv_variant_has_dual(int variant) { return variant == 0 || variant == 4 || (variant >= 6 && variant <= 9); }
int launch_spmv(const CsrView &A, int mode, const SpmvArgs &a, int variant, hipStream_t s);
int launch_spmv_dict(const CsrView &A, int mode, const SpmvArgs &a, int grid, hipStream_t s);
int launch_spmv_pattern(const CsrView &A, int mode, const SpmvArgs &a, int grid, hipStream_t s);
int launch_spmv_pair(const CsrView &A, int mode, const SpmvArgs &a, int grid, hipStream_t s);
int launch_spmv_stream(const CsrView &A, int mode, const SpmvArgs &a, int grid, hipStream_t s, bool *done);
// the measurement variants of schwz_csr_spmv (tools/probes/spmv_variants.hip): null in the product library
typedef int (*SpmvProbeHook)(const CsrView &A, int mode, const SpmvArgs &a, int variant, int grid, hipStream_t s);
extern SpmvProbeHook g_spmv_probe_hook;
// who may take the z-sweep walk (spmv_pair.hip): asked by launch_spmv_pair and by the plan of a CG solve
bool pair_sweep_update_ok(const CsrView &A, int grid, int diag_mode);  // kSpmvCgUpdate that leaves x alone
bool pair_sweep_dirdot_ok(const CsrView &A, int grid, int diag_mode);  // kSpmvDirDotSym
bool pair_sweep_start_ok(const CsrView &A, int grid);                  // start launch + first direction
bool pair_sweep_dual_ok(const CsrView &A, int grid);                   // ... with the fused check residual

// Jacobi scaling as the CG vector kernels see it.  The full 1/diag vector costs 8 B per row and
// per kernel; matrices with few distinct diagonal values (every stencil) get a 1-byte code per
// row into a <= 256-entry dictionary, or a single scalar.  Same values, same bits.
struct DiagView {
    int mode = 0;  // 0 none, 1 full vector, 2 dictionary codes, 3 uniform scalar
    const double *full = nullptr;
    const uint8_t *code = nullptr;
    const double *dict = nullptr;
    int ndict = 0;
    double uniform = 1.0;
};

// device-side CG scalar state
struct CgState {
    double rho[2];
    double rr;
    double r0;
    int iters;
    int stop_iter;
};

}  // namespace schwz

struct schwz_csr;
namespace schwz {
// plans the codings of the matrix (coding_plan.hpp: row patterns, then row pairs and the z-sweep walk, then the
// per-entry dictionaries), uploads what was accepted and binds it to A->v; the switches are read here, once
int build_spmv_dict(schwz_csr *A, const schwz_idx *h_rp, const schwz_idx *h_col, const double *h_val,
                    const std::vector<schwz_idx> &tiles);
struct CodingOptions;
struct HostCsr;
int build_spmv_pair(schwz_csr *A, const CodingOptions &opt, const HostCsr &M);
void free_spmv_pair(schwz_csr *A);
int pair_set_dual_split(schwz_csr *A, const schwz_idx *h_rp, const schwz_idx *h_col, int64_t split);
// marks the tiles whose rows or columns reach index >= split (see CsrView::tile_dual)
// host_setup.cpp (OpenMP): row_ptr monotone and every column in [0, ncols)
bool csr_is_well_formed(int64_t nrows, int64_t ncols, const schwz_idx *rp, const schwz_idx *col);
// host_setup.cpp (OpenMP): a_ij == a_ji bit for bit (rows with ascending columns)
bool csr_is_symmetric(int64_t nrows, int64_t ncols, const schwz_idx *rp, const schwz_idx *col, const double *val);
int csr_set_dual_split(schwz_csr *A, const schwz_idx *h_rp, const schwz_idx *h_col, int64_t split);
}  // namespace schwz

struct schwz_pcg;
namespace schwz {
// How a CG solve runs, every decision of it (cg.hip).  pcg_begin fills the part that follows from the matrix,
// the preconditioner and the switches and keeps it in schwz_pcg::plan; pcg_iterate completes its copy once
// rtol, max_iters and the outcome of the start launch are known.
struct CgPlan {
    bool general = false;       // block-Jacobi / ILU / ISAI: z = M^-1 r is an operator of its own
    bool qfree = false;         // row-pair coded matrix: q = A p is recomputed, never stored
    int dot_mode = kSpmvDot;    // launch that yields p.(A p)
    bool sweep_on = false;      // z-sweep walk of the update launch (where x is deferred)
    bool sweep_dirdot = false;  // ... and of the fused direction + p.(A p) launch
    bool fusedir = false;       // two launches per iteration
    bool deferx = false;        // x += sum alpha_k p_k applied once per kDeferDepth iterations
    bool sweep_start = false;   // the solve can start in the walk too (INIT / FIRST forms, spmv_pair.hip)
    bool initfold = false;      // ... and the FIRST launch then initialises CgState (no cg_init_finalize_kernel)
    int gs = 0, gv = 0;         // grids of the SpMV launches and of the vector kernels
    // completed by pcg_iterate
    bool walk_started = false;  // the start launch ran in the walk and left p to the first-direction launch
    bool p0_virtual = false;    // the first direction is never stored
    bool lazy_last = false;     // the update launch of the last iteration is postponed
    bool vlast = false;         // ... and its direction never stored
    bool graph = false;         // runs of kGraphIters iterations are replayed as a hipGraph
    int flavour = 0;            // what schwz_pcg_flavour reports (bits: schwz_pcg::last_flavour)
};
int pcg_begin(schwz_pcg *s, const double *d_b, double *d_x, double rtol, bool fused, const double *d_x2,
              int64_t row_limit, hipStream_t st);
int pcg_iterate(schwz_pcg *s, double *d_x, double rtol, int max_iters, hipStream_t st);
bool pcg_defers_x(schwz_pcg *s);  // the next solve would defer x (what schwz_pcg::x_out needs)
int precond_apply(schwz_pcg *s, const double *in, double *out, hipStream_t st);
int pcg_last_stats(schwz_pcg *s, int *h_iters, double *h_resnorm);  // device sync + state copy
int pcg_take_trs_error(schwz_pcg *s);
// the checks of schwz_pcg_create_ilu on the ParILU options (SCHWZ_OK, SCHWZ_ERR_INVALID or
// SCHWZ_ERR_NOT_IMPLEMENTED, message set)
int pcg_check_ilu_sweeps(int precond, int par_ilu_sweeps, int trisolve_sweeps);
int pcg_create_impl(const schwz_csr *A, int precond, int block_size, int par_ilu_sweeps, int trisolve_sweeps,
                    schwz_pcg **out);
// The two Krylov solvers of the non-symmetric branch (gmres.hip, bicgstab.hip) around a preconditioner object they
// take over (on failure it stays the caller's), the object a solver holds, and giving it up before the solver is
// destroyed: schwz_ras_set_nonsym_solver hands the preconditioner from one solver to the other.
int gmres_create_adopt(const schwz_csr *A, int restart, int basis, schwz_pcg *pre, schwz_gmres **out);
schwz_pcg *gmres_precond(schwz_gmres *s);
schwz_pcg *gmres_release_precond(schwz_gmres *s);
int bicgstab_create_adopt(const schwz_csr *A, schwz_pcg *pre, schwz_bicgstab **out);
schwz_pcg *bicgstab_precond(schwz_bicgstab *s);
schwz_pcg *bicgstab_release_precond(schwz_bicgstab *s);
int pcg_finish_lazy(schwz_pcg *s);  // the postponed residual update / state advance of the last solve, if any  // ILU(0) sweeps: trs_take_error of the factor solves
// schwz_ras_restart: what a solver object remembers of its last solve -- postponed launches and their saved stream,
// second outputs, pending norms, the state schwz_ras_last_inner_stats reads -- is forgotten, as after creation;
// nothing postponed is run.  The device state is zeroed on `st`.  A null solver is fine.
int pcg_forget(schwz_pcg *s, hipStream_t st);
int pcg_f32_forget(schwz_pcg_f32 *s, hipStream_t st);
int cheb_forget(schwz_cheb *s, hipStream_t st);
int gmres_forget(schwz_gmres *s, hipStream_t st);
int bicgstab_forget(schwz_bicgstab *s, hipStream_t st);
}  // namespace schwz

// ---- opaque ABI types -------------------------------------------------------

struct schwz_csr {
    schwz::CsrView v;
    // (every device array frees itself: schwz_csr_destroy is `delete`)
    schwz::Dev<schwz_idx> d_rp, d_col, d_tile, d_wtile, d_order, d_tile_nz, d_stream_order;
    schwz::Dev<double> d_val;
    // device arrays of the codings, one struct per plan of coding_plan.hpp (uploaded and bound to `v` by
    // spmv_dict.hip / spmv_pair.hip)
    struct Coding {
        struct { schwz::DevBuf pat_id, tile_table, tbl_desc, tbl_len, tbl_val, tbl_delta; } pattern;
        struct { schwz::DevBuf code, vptr, dptr, vdict, ddict; } dict;
        struct { schwz::DevBuf pair_id, rle, chunk_ptable, ptbl_desc, ptbl_len, ptbl_val, ptbl_meta; } pair;
        struct {
            schwz::DevBuf gen, chain_plane, chain_far, rec, rec_dir, rec_first, canon_ready, canon_sym_ready;
        } walk;
        struct { schwz::DevBuf chunk_dual, chain_dual, dual_chunks; } dual;
    } coding;
    schwz::Dev<uint8_t> d_tile_dual;
    std::vector<int> h_chain_plane;  // host copy of CsrView::chain_plane (z-sweep walk built)
    std::vector<schwz_idx> h_tiles;  // host copy of the tile boundaries
    int pair_deal_shift = 0;         // log2 of the run length (in tiles) of the XCD deal the pair kernels derive theirs from
    double dict_fraction = 0.0;  // share of the nonzeros that are dictionary coded
    double pattern_fraction = 0.0;  // share of the nonzeros in row-pattern coded tiles
    double pair_fraction = 0.0;     // share of the nonzeros in row-pair coded tiles
    int64_t pair_code_bytes = 0;    // pattern ids (run-length or byte form) + chunk table ids + tables of the pair coding
};

struct schwz_pcg {
    const schwz_csr *A = nullptr;
    int precond = 0;
    int64_t n = 0;
    // (every device buffer, event and stream below frees itself: schwz_pcg_destroy lists none of them)
    schwz::Dev<double> r, p, q, dinv;
    schwz::Dev<double> r_alt;  // second residual buffer of the virtual first direction (cg.hip: r1 goes there, r0 stays)
    // general preconditioners (block-Jacobi, ILU(0)): z = M^-1 r is a vector of its own
    schwz::Dev<double> z;
    int block_size = 1;
    schwz::Dev<schwz_idx> d_blk_id;  // block-Jacobi: index of each block's inverse
    schwz::Dev<double> d_blk_inv;    // unique inverse blocks, [nunique][bs][bs] (a k x k inverse in the top left corner)
    schwz::Dev<schwz_idx> d_row_blk, d_blk_ptr;  // detected blocks of different sizes: block of a row, boundaries
    // (the three adopted objects: schwz_pcg_destroy destroys them)
    schwz_trs *ilu = nullptr;       // ILU(0): level-scheduled L and U sweeps
    int par_ilu_sweeps = 0;         // ILU / ISAI factors from this many ParILU sweeps (0: exact host ILU(0))
    int trisolve_sweeps = 0;        // ILU applied by this many Jacobi passes per factor (0: exact solves)
    schwz_csr *isai_l = nullptr, *isai_u = nullptr;  // ISAI: approximate inverses of L and U
    schwz::Dev<double> isai_tmp;
    schwz::DiagView diag;
    schwz::DevBuf d_dcode, d_ddict;
    schwz::Dev<double> partials;  // 3 * kMaxGrid (SpMV banks) + 2 * kMaxGrid (vector banks) + 3 * kMaxGrid (start banks, InitFold)
    schwz::Dev<double> stream_part;  // SpmvArgs::stream_part of this solver's launches (and of the GMRES / BiCGSTAB around it)
    schwz::Dev<double> norm_sq_own;
    double *d_norm_sq = nullptr;  // kSpmvResidDual result: norm_sq_own, or for one start launch the caller's (subdomain.hip)
    schwz::StateMirror<schwz::CgState> state;  // device state, pinned mirror, poll (solver_state.hpp)
    int variant = 0;
    // recorded runs of kGraphIters iterations (launch-bound small systems), see pcg_iterate
    struct Captured {
        double *x;
        double rtol;
        int variant;
        int flavour;  // CgPlan::flavour of the solve that recorded it (which launches the graph holds)
        schwz::GraphExec exec;
    };
    std::vector<Captured> graphs;
    schwz::Stream capture_stream;
    // deferred x update of large systems (pcg_iterate): ring of search directions and their alphas
    schwz::Dev<double> p_ring;      // kDeferDepth - 2 vectors; slots 0 and 1 of the ring are p and q
    schwz::Dev<double> alpha_hist;  // kDeferDepth
    bool ring_failed = false;
    bool ring_has_q = true;  // slot 1 of the ring is s->q (q-free iteration); false: the stored-q iteration's ring
    // the start launch of the running solve left p to the first fused direction launch (z-sweep start)
    bool p_pending = false;
    schwz::CgPlan plan;  // of the running solve, as far as pcg_begin decides it
    // Rows the caller wants final FIRST (a subdomain's boundary rows, which its neighbours wait for): the
    // last x update of a solve takes [0, prio_lo) and [prio_hi, n) ahead of the rest and records prio_event
    // in between, so that the halo pack + send can run beside the remaining update (schwz_ras_pack_early).
    // Without a deferred x update the event is recorded behind the last launch of the solve.
    bool prio_on = false;
    // Second output of the LAST x update of a solve (cg_flush_x_kernel): rows [0, x2_rows) of the result also go
    // to x2_out -- the restriction x~[interior] = y[interior] without a launch of its own.  x2_written: the last
    // solve did write it (deferred x update; otherwise the caller copies).
    double *x2_out = nullptr;
    int64_t x2_rows = 0;
    const double *x2_src = nullptr;  // rows [x2_rows, x2_total) of x2_out are copied from here (overlap / halo of x~)
    int64_t x2_total = 0;
    bool x2_written = false;
    // A result vector of its own: the solve reads its start vector d_x, leaves it untouched and stores the result
    // here (the first x update of the solve runs out of place, the later ones in place on x_out).  Only with the
    // deferred x update -- pcg_iterate refuses otherwise, pcg_defers_x tells beforehand -- and not together with the
    // priority-row split, which exists only on subdomains with neighbours, where nobody sets it.
    double *x_out = nullptr;
    // The start launch of the running solve left its partial sums to the first-direction launch (CgPlan::initfold):
    // what that launch -- or, where none follows, cg_init_finalize_kernel from pcg_iterate -- folds, and the
    // event pcg_iterate records once CgState and the check norm are final (the caller sets it, one solve at a time).
    struct InitFold {
        bool pending = false;
        const double *partials = nullptr;
        int nparts = 0;
        double rtol = 0.0;
        double *norm_sq_out = nullptr;
        int norm_bank = 1;
    } init;
    hipEvent_t init_event = nullptr;  // borrowed
    // A solve of exactly max_iters iterations (rtol == 0) whose last iteration was cut down to what its result
    // needs: alpha of that iteration is formed inside the x update, and the residual update + state advance --
    // whose results nothing reads unless the caller asks for the iteration count / residual norm -- wait in
    // `lazy` until pcg_finish_lazy runs them (pcg_last_stats, schwz_pcg_solve with outputs) or the next solve
    // drops them.
    struct LazyLast {
        bool pending = false;
        hipStream_t stream = nullptr;  // borrowed
    } lazy;
    std::function<int(hipStream_t)> lazy_run;
    int64_t prio_lo = 0, prio_hi = 0;  // even
    schwz::Event prio_event;
    // how the last solve iterated: bits 0-1: 0 stored q, 1 q-free (three launches), 2 q-free with the fused
    // direction + p.(A p) launch; 4: deferred x update; 8: z-sweep walk of the update launch; 16: of the fused launch;
    // 32: of the start launch and the first direction as well; 64 / 128: first / last direction never stored
    int last_flavour = 0;
};

struct schwz_trs {
    int64_t n = 0;
    // (every device array, the capture stream and the graphs free themselves: schwz_trs_destroy is `delete`)
    schwz::Dev<schwz_idx> l_rp, l_col, u_rp, u_col;
    schwz::Dev<double> l_val, u_val;
    // w[i] = b[perm[i]] before the sweeps, y[perm_out[i]] = w[i] after them: the same array for LL^T and
    // ILU (perm_out points at perm), the row and the column permutation of an LU (schwz_trs_create_lu: perm_out
    // points at perm_col)
    schwz::Dev<schwz_idx> perm, perm_col;
    const schwz_idx *perm_out = nullptr;  // borrowed
    // level schedules: rows sorted by level, level pointers
    schwz::Dev<schwz_idx> l_order, l_lvl, u_order, u_lvl;
    int l_nlvl = 0, u_nlvl = 0;
    schwz::Dev<double> w0, w1;
    // launch plan for factors too large for the one-workgroup kernel: runs of narrow levels
    // (one workgroup, barriers in between) and wide levels (one multi-workgroup launch each)
    struct Seg {
        int lvl0, lvl1;
        bool wide;
    };
    std::vector<Seg> l_plan, u_plan;
    std::vector<schwz_idx> h_l_lvl, h_u_lvl;
    bool fused = true;  // whole solve in the single-workgroup kernel
    // multi-launch plan as hipGraphs, one per (b, y) pair it has been asked for: a sweep over a
    // 256^3 subdomain is ~1500 tiny launches, replayed as ONE graph launch
    struct Captured {
        const double *b;
        double *y;
        schwz::GraphExec exec;
    };
    std::vector<Captured> graphs;
    schwz::Stream capture_stream;
    bool graphs_failed = false;  // capture / instantiate refused once: launch by launch from then on
    // flag-driven sweeps (trs_flag_kernel): the two solution vectors that double as per-row flags
    bool flags = false;
    schwz::Dev<unsigned long long> f0, f1;
    schwz::Dev<int> d_err;
    // the factors in level order (rows at their position in the level-sorted order, columns = positions)
    schwz::Dev<schwz_idx> fl_rp, fl_col, fu_rp, fu_col;
    schwz::Dev<double> fl_val, fu_val;
    schwz::Dev<schwz_idx> fl_src, fu_src, fu_dst;  // rhs gather / y scatter per position
    int flag_grid = 0;
    // LU factors (schwz_trs_create_lu) with rows beyond one lane each: trs_flag_wave_kernel, one wave per row
    bool wave = false;
    // Jacobi-sweep mode (schwz_trs_create_sweeps, csrc/parilu.hip): `sweeps` passes per factor over the strict
    // parts (CSR) with the reciprocal diagonals; w0, w1, w2 double-buffer the passes.  0: exact solves.
    int sweeps = 0;
    schwz::Dev<schwz_idx> js_l_rp, js_l_col, js_u_rp, js_u_col;
    schwz::Dev<double> js_l_val, js_u_val, js_l_dinv, js_u_dinv;
    schwz::Dev<double> w2;
};

namespace schwz {
// y = U^-1 L^-1 b in the Jacobi-sweep mode of schwz_trs (csrc/parilu.hip)
int trs_sweeps_solve(schwz_trs *t, const double *b, double *y, hipStream_t st);
// ParILU factors of the matrix whose pattern h_rp / h_col is and whose values d_val hold (HBM), with the values
// copied back to malloc'd host arrays (csrc/parilu.hip)
int parilu_host_factors(int64_t n, const schwz_idx *h_rp, const schwz_idx *h_col, const double *d_val, int sweeps,
                        schwz_idx **l_rp, schwz_idx **l_col, double **l_val, schwz_idx **u_rp, schwz_idx **u_col,
                        double **u_val);
}  // namespace schwz

// host-side global problem (explicit CSR or analytic stencil)
struct schwz_problem {
    int kind = 0;  // 0 csr, 1 csr rows of a subset of the rows (distributed ingest), 2 lap2d, 3 lap3d
    // kind 1: the global ids of the rows this process holds, ascending; rp / col / val cover those rows in
    // that order.  Asking for another row is an error of the caller: row() returns 0 entries and notes it.
    std::vector<int64_t> present;
    mutable int64_t missing_row = -1;
    int64_t N = 0;
    int64_t nx = 0, ny = 0, nz = 0;
    std::vector<int64_t> rp;
    std::vector<schwz_idx> col;
    std::vector<double> val;
    int64_t nnz() const;
    // writes up to 16 (stencil) or row-length entries; returns count
    int row(int64_t g, int64_t *cols, double *vals) const;
    int max_row_nnz = 0;
};

struct schwz_pcg_f32;  // cg_f32.hip
struct schwz_cheb;     // chebyshev.hip

// ---- aggregation coarse correction (coarse.hip; the plan is coarse_plan.hpp's) ----
// one per process / device: the explicit inverse of A0 = Z^T A Z, the coarse residual s and the correction c
struct schwz_coarse {
    int32_t nc = 0;
    schwz::Dev<double> inv, s, c;
};

// a subdomain's part, uploaded by schwz_ras_coarse_set_aggregates
struct schwz_coarse_part {
    int32_t first_agg = 0, m = 0, nc = 0, npieces = 0;
    int64_t nslots = 0, nw = 0;
    schwz::Dev<double> beta, w_val, partial;
    schwz::Dev<int32_t> w_slot, piece, piece_ptr;  // piece: {aggregate, begin, end} per piece
    schwz::Dev<uint16_t> id16;
    std::vector<double> rows;  // m x nc: the subdomain's rows of A0 (schwz_ras_coarse_rows)
    // schwz_ras_rhs_aggregate (rhs.hip) and schwz_ras_aggregate_sums (coarse.hip), built by ensure_agg_rows at the first
    // call of either: the interior rows grouped by aggregate, ascending inside each (agg_rows, 4 B per interior row),
    // aggregate a's rows at [agg_ptr[a], agg_ptr[a + 1]); for aggregate_sums their cut into pieces of at most
    // kCoarsePieceCap rows (row_piece: {aggregate, begin, end} per piece, row_piece_ptr: m + 1) and a partial sum per piece
    schwz::Dev<int32_t> agg_rows, agg_ptr, row_piece, row_piece_ptr;
    schwz::Dev<double> row_partial;
    int32_t nrow_pieces = 0;
    bool agg_ready = false;
};

namespace schwz {
// the tables above from the slot ids the coarse part holds in HBM: planned on the host (coarse_plan.cpp), uploaded on
// `st`, which is waited for; nothing to do after the first call
int ensure_agg_rows(schwz_subdomain *sd, hipStream_t st);
// x[j] += c[id16[j]] over nx slots and, where y is a buffer of its own (not null), y[j] += c[id16[j]] over ny <= nx
int launch_coarse_apply(const schwz_coarse_part *part, const schwz_coarse *c, double *x, int64_t nx, double *y, int64_t ny,
                        hipStream_t st);
}  // namespace schwz

namespace schwz {
// The solver the next local solve of a subdomain runs: local_kind (subdomain.hip) decides it, and everything that
// depends on the solver switches over it.  A new solver adds one enumerator and one case per switch.
enum class LocalKind { Direct, Gmres, Bicgstab, CgF32, Chebyshev, Cg };
}  // namespace schwz

struct schwz_subdomain {
    // ---- host index sets -------------------------------------------------
    int P = 0, me = 0, overlap = 0;
    int64_t N = 0;
    std::vector<int64_t> first_row;
    int64_t local_size = 0, local_size_x = 0, overlap_size = 0, halo_size = 0;
    std::vector<int64_t, schwz::NoInitAlloc<int64_t>> l2g;  // local_size_x + halo (interior part filled by all threads)
    std::unordered_map<int64_t, schwz_idx> g2l_x;  // non-interior global -> local
    // (col / val: no value-initialisation on resize -- every entry is written by the threads that fill the matrix,
    // which also places the pages near them)
    std::vector<schwz_idx, schwz::NoInitAlloc<schwz_idx>> l_rp;
    std::vector<schwz_idx, schwz::NoInitAlloc<schwz_idx>> l_col;
    std::vector<double, schwz::NoInitAlloc<double>> l_val;
    std::vector<schwz_idx, schwz::NoInitAlloc<schwz_idx>> i_rp;  // interface rows (local_size_x+1)
    std::vector<int64_t> i_col_global;
    std::vector<double> i_val;
    std::vector<int> nbr_in, nbr_out;
    std::vector<std::vector<int64_t>> get, put;  // global ids
    int64_t num_recv = 0, num_send = 0;
    schwz_idx to_local(int64_t g) const
    {
        if (g >= first_row[me] && g < first_row[me + 1]) return (schwz_idx)(g - first_row[me]);
        auto it = g2l_x.find(g);
        return it == g2l_x.end() ? -1 : it->second;
    }
    // ---- device state -----------------------------------------------------
    // Everything in HBM, and every object that owns HIP resources, lives in schwz_subdomain_device (below), reached
    // through this one plain pointer: null until schwz_subdomain_to_device, deleted by schwz_subdomain_destroy.
    // "On the device" is `dev != nullptr`.  (A pointer, not a member: host_setup.cpp and the host-only test drivers
    // create and delete subdomains in programs linked without the HIP runtime, so no destructor that frees device
    // memory may be reachable from ~schwz_subdomain.)
    struct schwz_subdomain_device *dev = nullptr;
    schwz_solver_options opt{};
    int gmres_basis = 0;  // SCHWZ_GMRES_BASIS_*: the basis type of dev->gmres, and of the one a return from bicg creates
    int precision = 0;    // schwz_ras_set_local_precision
    int sym_solver = 0;   // schwz_ras_set_sym_solver
    int64_t nnz_interface = 0;
    // schwz_ras_rhs_gather (rhs.hip): the global position of every local row's right-hand side.  rhs_index holds the
    // caller's map (schwz_ras_rhs_index; empty: l2g itself); the device copy is made at the first gather, not before
    std::vector<int64_t> rhs_index;
    bool rhs_index_custom = false;
};

// block state of a subdomain (schwz_ras_batch_begin, csrc/batch.hip): k right-hand sides at once, vectors and a solver
// of its own.  Nothing of the subdomain is read-write shared with it: it reads the matrix and the index lists
struct schwz_ras_batch {
    int k = 0;
    schwz_bcg *cg = nullptr;
    schwz::Dev<double> x, rhs, bt, y;
    ~schwz_ras_batch() { schwz_bcg_destroy(cg); }
};

// The device half of a subdomain.  Every buffer, the pinned scalar and the event free themselves; the destructor
// (subdomain.hip) destroys the matrix and the adopted solver objects through their schwz_*_destroy functions and
// deletes `coarse` and `batch`.  Only .hip translation units may create or delete one.
struct schwz_subdomain_device {
    schwz_subdomain_device() = default;
    schwz_subdomain_device(const schwz_subdomain_device &) = delete;
    ~schwz_subdomain_device();
    schwz_csr *A = nullptr;  // local_matrix
    // The solver objects.  Which of them the next local solve runs is local_kind's answer (subdomain.hip); nothing
    // else chooses a path by these pointers or by `precision` / `sym_solver`.
    schwz_pcg *cg = nullptr;       // symmetric local matrix, iterative (LocalKind::Cg, and the two below beside it)
    schwz_gmres *gmres = nullptr;  // non-symmetric local matrix (Gmres)
    schwz_bicgstab *bicg = nullptr;  // ... once schwz_ras_set_nonsym_solver asked for BiCGSTAB (Bicgstab; gmres is null then)
    // mixed-precision local solve (schwz_ras_set_local_precision, csrc/cg_f32.hip): created at first use, CgF32 while
    // `precision` is SCHWZ_PRECISION_F32; `cg` stays what it is, so that F64 restores the fp64 path exactly
    schwz_pcg_f32 *cg32 = nullptr;
    // Chebyshev local solve (schwz_ras_set_sym_solver, csrc/chebyshev.hip): created at first use, Chebyshev while
    // `sym_solver` is SCHWZ_SYM_CHEBYSHEV; `cg` stays what it is, so that SCHWZ_SYM_CG restores the CG path exactly
    schwz_cheb *cheb = nullptr;
    schwz_trs *trs = nullptr;  // the direct solvers' factors (Direct)
    // interface rows: only overlap rows are non-empty; stored compactly
    schwz::Dev<schwz_idx> d_i_rp, d_i_col;  // cols index x~ directly
    schwz::Dev<double> d_i_val;
    schwz::Dev<schwz_idx> d_put_idx, d_get_idx;  // local ids, packed
    schwz::Dev<double> d_x;       // x~ [interior|overlap|halo]
    schwz::Dev<double> d_x_alt;   // the other x~ buffer: the last x update of a CG solve writes its interior, the restriction swaps the two
    schwz::Dev<double> d_rhs;     // b_loc
    schwz::Dev<double> d_btilde;  // b~ = local_solution on entry of the solve
    schwz::Dev<double> d_y;       // init_guess / solve result of the separate form (allocated at first need)
    // Unified form (subdomain.hip, want_unified): no overlap, no halo, CG with x deferred -- y and x~ are the same n
    // values, and y lives in one of the two x~ buffers.  State A: y IS x~ (d_x).  State B (y_in_alt): y is d_x_alt,
    // after a solve that has not been restricted.
    bool unified = false;
    bool y_in_alt = false;
    // separate form: a solve has run since the last restriction (y is ahead of x~)
    bool y_ahead = false;
    schwz::Dev<double> d_partials;
    schwz::Dev<double> d_stream_part;  // SpmvArgs::stream_part of the subdomain's own norm launches
    schwz::Pinned<double> h_scalar;  // mapped
    double *d_h_scalar = nullptr;    // device alias of h_scalar (borrowed)
    schwz::Event ev_scalar;
    // aggregation coarse correction (schwz_ras_coarse_set_aggregates); null: one-level RAS, nothing of it runs
    schwz_coarse_part *coarse = nullptr;
    schwz::Dev<int64_t> d_rhs_index;  // device copy of the map of schwz_ras_rhs_gather (schwz_subdomain::rhs_index)
    schwz_ras_batch *batch = nullptr;  // null until asked for
    // schwz_ras_apply_interior on a subdomain with overlap rows: A x~ on all local_size_x rows (allocated at first need)
    schwz::Dev<double> d_apply;
};

namespace schwz {
// rhs.hip: one pass that puts the vectors of a subdomain back to what the upload left -- x (nx entries) and, where
// they exist, x_alt (nx) and y (n) zero, bt[0:n] = b[0:n]
int launch_restart(int64_t n, int64_t nx, const double *b, double *bt, double *x, double *x_alt, double *y, hipStream_t st);
}  // namespace schwz

namespace schwz {
int trs_take_error(schwz_trs *t);  // trs.hip: SCHWZ_ERR_HIP (and the reason) if a flag-driven sweep timed out
}
