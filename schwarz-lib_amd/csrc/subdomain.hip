// Device-resident RAS iteration of one subdomain: the five steps of
// SchwarzBase::run (source/schwarz_base.cpp:387-452) as stream-ordered launches.
//
// HBM layout per subdomain (one GPU):
//   x~      [interior | overlap | halo]  doubles   -- replaces the N-long
//           global_solution of the reference (schwarz_base.cpp:340-341)
//   A_loc   CSR over [interior|overlap] rows and columns, int32 indices
//   A_Gamma CSR over the overlap rows only, columns index x~ directly
//   b_loc, b~, y (CG warm start), r, p, q, 1/diag : local_size_x doubles each
//           (y: a vector of its own, or -- unified form, below -- one of the two x~ buffers)
//   put / get lists: int32 local ids, packed in neighbour order
// All of it belongs to schwz_subdomain_device (schwz_internal.hpp), which the subdomain reaches through sd->dev:
// the buffers free themselves, its destructor (below) destroys the matrix and the solver objects, and
// schwz_subdomain_destroy deletes it.  sd->dev is null on a host-only subdomain.
#include <hip/hip_runtime.h>

#include <cstring>

#include <cmath>

#include "schwz_internal.hpp"

using namespace schwz;

// ---- where the solver's vector y lives -----------------------------------------------------------------------
// On a subdomain without overlap and without halo (one subdomain) y and x~ are the same local_size_x values: the
// check residual is the CG start residual, and the restriction copies all of y.  When the local solver is CG with
// the deferred x update, y then needs no memory of its own (UNIFIED form):
//   state A  y IS x~ (d_x): after the upload and after every restriction.  A solve reads its start vector from d_x,
//            leaves d_x untouched -- a discarded solve must not change x~ -- and stores its result to d_x_alt
//            (schwz_pcg::x_out: one store of the solution instead of two) -> state B
//   state B  y is d_x_alt.  The restriction swaps the buffers -> state A.  Another solve first (a discarded one
//            before it, or schwz_ras_local_solve twice) runs in place on y, and its check residual, on x~, is no
//            longer its start residual: the separate launches.
// Everything else is the SEPARATE form: y = d_y, the restriction swaps (schwz_pcg::x2_out) or copies.  The form is
// chosen per solve (the switches are read per solve); a change of form carries y over with one copy.  With
// neighbours (overlap or halo entries, the priority-row split of the last x update) the form is always separate.
//
// ---- which solver the next local solve runs ------------------------------------------------------------------
// The one place that reads opt.local_solver, gmres, bicg, precision and sym_solver to decide it.  It relies on:
//   - precision == F32 and sym_solver == CHEBYSHEV exclude each other: each setter refuses while the other is set;
//   - both need cg (the setters' eligibility test) and have created cg32 / cheb before they set the field;
//   - gmres and bicg exclude each other and exclude cg: create_local_solver makes gmres or cg, and
//     schwz_ras_set_nonsym_solver replaces one of gmres / bicg by the other.
// (Cg is also the answer of an iterative subdomain whose solver could not be created: who takes that path checks cg.)
// Only Cg has the unified form, the restriction by the solver, the fused check + start residual, the boundary
// event of pack_early and a flavour; the other kinds update d_y in place (solve_in_place).
static LocalKind local_kind(const schwz_subdomain *sd)
{
    if (sd->opt.local_solver != SCHWZ_SOLVER_ITERATIVE) return LocalKind::Direct;
    if (sd->dev && sd->dev->gmres) return LocalKind::Gmres;
    if (sd->dev && sd->dev->bicg) return LocalKind::Bicgstab;
    if (sd->precision == SCHWZ_PRECISION_F32) return LocalKind::CgF32;
    if (sd->sym_solver == SCHWZ_SYM_CHEBYSHEV) return LocalKind::Chebyshev;
    return LocalKind::Cg;
}

static int local_maxit(const schwz_subdomain *sd)
{
    return sd->opt.local_max_iters == -1 ? (int)sd->local_size_x : sd->opt.local_max_iters;
}

// SCHWZ_RESTRICT_FUSE=0: y in a vector of its own and the restriction as a copy launch (read per solve: tests switch it)
static bool restrict_fuse_on()
{
    const char *e = std::getenv("SCHWZ_RESTRICT_FUSE");
    return !(e && e[0] == '0');
}

static bool want_unified(schwz_subdomain *sd)
{
    schwz_subdomain_device *d = sd->dev;
    return local_kind(sd) == LocalKind::Cg && d->cg && restrict_fuse_on() && sd->overlap_size == 0 &&
           sd->halo_size == 0 && sd->local_size > 0 && !d->cg->prio_on && pcg_defers_x(d->cg);
}

// the second x~ buffer, allocated at first need (zeroed); false: no room
static bool ensure_x_alt(schwz_subdomain *sd)
{
    Dev<double> &alt = sd->dev->d_x_alt;
    if (alt) return true;
    if (alt.alloc((size_t)std::max<int64_t>(sd->local_size_x + sd->halo_size, 1), true)) {
        (void)hipGetLastError();
        alt = Dev<double>();
        return false;
    }
    return true;
}

static double *y_of(const schwz_subdomain *sd)
{
    const schwz_subdomain_device *d = sd->dev;
    return d->unified ? (d->y_in_alt ? d->d_x_alt : d->d_x) : d->d_y;
}

// the form of the solve about to be launched; y moves with one copy where it differs from the current one
static int choose_form(schwz_subdomain *sd, hipStream_t st)
{
    const bool uni = want_unified(sd) && ensure_x_alt(sd);
    schwz_subdomain_device *d = sd->dev;
    if (uni == d->unified) return SCHWZ_OK;
    const int64_t n = sd->local_size_x;
    int rc;
    if (uni) {
        // y ahead of x~ (a solve that was not restricted): state B.  Otherwise state A, where y is x~: the copy makes
        // it so even where the caller wrote into y -- which the separate form, too, takes for x~ in its check residual.
        if ((rc = launch_copy(n, d->d_y, d->y_ahead ? d->d_x_alt : d->d_x, st))) return rc;
        d->y_in_alt = d->y_ahead;
    } else {
        if (!d->d_y && (rc = d->d_y.alloc((size_t)(n ? n : 1), true))) return rc;
        if ((rc = launch_copy(n, y_of(sd), d->d_y, st))) return rc;
        d->y_ahead = d->y_in_alt;
        d->y_in_alt = false;
    }
    d->unified = uni;
    return SCHWZ_OK;
}

// One fp64 CG solve in the form choose_form has just settled; solve(y) launches it.  Unified: state A out of place,
// d_x -> d_x_alt, state B in place on d_x_alt.  Separate: in place on d_y, with step 4 inside step 3 -- the last x
// update also writes the interior rows into the OTHER x~ buffer (schwz_pcg::x2_out) and copies the overlap / halo
// entries of the current one behind them, and schwz_ras_restrict then only swaps the two buffers.  A solve that is
// discarded (the verdict was "converged": no restriction) leaves the current buffer untouched, like the reference,
// which breaks before the solve.  The second buffer is allocated on first use; SCHWZ_RESTRICT_FUSE=0 keeps the copy.
template <typename Solve>
static int cg_solve_in_form(schwz_subdomain *sd, Solve solve)
{
    schwz_subdomain_device *d = sd->dev;
    schwz_pcg *cg = d->cg;
    cg->x2_out = nullptr;
    if (d->unified) {
        cg->x_out = d->y_in_alt ? nullptr : d->d_x_alt;
    } else {
        d->y_ahead = true;
        if (restrict_fuse_on() && sd->local_size > 0 && ensure_x_alt(sd)) {
            cg->x2_out = d->d_x_alt;
            cg->x2_rows = sd->local_size;
            cg->x2_src = d->d_x;
            cg->x2_total = sd->local_size_x + sd->halo_size;
        }
    }
    const int rc = solve(y_of(sd));
    cg->x_out = nullptr;
    if (d->unified && !rc) d->y_in_alt = true;
    return rc;
}

// The kinds without a form of their own: y = d_y updated in place, the restriction is the copy launch.  (A BiCGSTAB
// breakdown simply ends this local solve: the next outer iteration starts again from y with a fresh rhat.)
static int solve_in_place(schwz_subdomain *sd, int *h_iters, schwz_stream stream)
{
    schwz_subdomain_device *d = sd->dev;
    if (d->cg) {
        const int rc = choose_form(sd, (hipStream_t)stream);  // -> separate: want_unified is false for these kinds
        if (rc) return rc;
        d->cg->x2_out = nullptr;
        d->cg->x2_written = false;  // (or schwz_ras_restrict would swap in a stale buffer)
    }
    d->y_ahead = true;
    const double tol = sd->opt.local_tol;
    const int maxit = local_maxit(sd);
    switch (local_kind(sd)) {
    case LocalKind::Direct:
        if (h_iters) *h_iters = 0;
        return schwz_trs_solve(d->trs, d->d_btilde, d->d_y, stream);
    case LocalKind::Gmres: return schwz_gmres_solve(d->gmres, d->d_btilde, d->d_y, tol, maxit, h_iters, nullptr, stream);
    case LocalKind::Bicgstab: return schwz_bicgstab_solve(d->bicg, d->d_btilde, d->d_y, tol, maxit, h_iters, nullptr, stream);
    case LocalKind::CgF32: return schwz_pcg_f32_solve(d->cg32, d->d_btilde, d->d_y, tol, maxit, h_iters, nullptr, stream);
    case LocalKind::Chebyshev: return schwz_cheb_solve(d->cheb, d->d_btilde, d->d_y, tol, maxit, h_iters, nullptr, stream);
    case LocalKind::Cg: break;  // not in place: schwz_ras_local_solve takes it through cg_solve_in_form
    }
    return SCHWZ_ERR_INVALID;
}

// Rows the neighbours wait for (the put lists: interior rows next to the subdomain boundary) become final ahead of
// the rest of the solution, so that the next halo exchange can start beside the tail of the solve
// (schwz_ras_pack_early).  Two ranges [0, lo) and [hi, n) around the widest gap of the sorted put ids `ids`; false:
// no put id, or one beyond the interior (no split at all).
static bool priority_rows(const std::vector<schwz_idx> &ids, int64_t n, int64_t local_size, int64_t *lo_out, int64_t *hi_out)
{
    if (ids.empty() || ids.back() >= local_size) return false;
    int64_t lo = 0, hi = n, gap = -1, prev = -1;
    for (size_t k = 0; k <= ids.size(); ++k) {
        const int64_t cur = k < ids.size() ? (int64_t)ids[k] : n;
        if (cur - prev > gap) {
            gap = cur - prev;
            lo = prev + 1;
            hi = cur;
        }
        prev = cur;
    }
    lo = (lo + 1) & ~int64_t(1);
    hi = hi & ~int64_t(1);
    if (hi < lo) hi = lo;
    // (put lists spread over more than a quarter of the rows, an irregular partition: no split, the event follows
    // the whole update and the exchange overlaps the restriction only)
    const bool split = lo + (n - hi) <= n / 4;
    *lo_out = split ? lo : (n & ~int64_t(1));
    *hi_out = split ? hi : (n & ~int64_t(1));
    return true;
}

// the solver object of sd->opt around sd->dev->A: what local_kind then finds
static int create_local_solver(schwz_subdomain *sd, std::vector<schwz_idx> put_idx)
{
    schwz_subdomain_device *d = sd->dev;
    const schwz_solver_options &o = sd->opt;
    const int64_t n = sd->local_size_x;
    int rc;
    if (o.local_solver == SCHWZ_SOLVER_ITERATIVE) {
        const int bsz = o.precond_block_size < 1 ? 1 : o.precond_block_size;
        // solve.cpp:486-520: GMRES(restart_iter); the preconditioner objects are the CG's
        if (o.non_symmetric)
            return schwz_gmres_create_ex(d->A, o.precond, bsz, o.restart_iter < 1 ? 1 : o.restart_iter, o.par_ilu_sweeps,
                                         o.trisolve_sweeps, &d->gmres);
        if ((rc = o.par_ilu_sweeps || o.trisolve_sweeps
                      ? schwz_pcg_create_ilu(d->A, o.precond, o.par_ilu_sweeps, o.trisolve_sweeps, &d->cg)
                      : schwz_pcg_create_ex(d->A, o.precond, bsz, &d->cg)))
            return rc;
        d->cg->variant = o.spmv_variant;
        std::sort(put_idx.begin(), put_idx.end());
        if (priority_rows(put_idx, n, sd->local_size, &d->cg->prio_lo, &d->cg->prio_hi)) {
            if ((rc = d->cg->prio_event.create())) return rc;
            d->cg->prio_on = true;
        }
        return SCHWZ_OK;
    }
    // factorization == "umfpack": P A Q = L U on the host, the triangular solves with both permutations on the GPU
    // (solve.cpp:144-173,253-267,321-390); else Solve::compute_local_factors + the Ginkgo TRS setup
    // (solve.cpp:75-143,281-399), L L^T with one permutation
    const bool lu = o.local_solver == SCHWZ_SOLVER_DIRECT_LU;
    schwz_idx *l_rp = nullptr, *l_col = nullptr, *u_rp = nullptr, *u_col = nullptr, *perm = nullptr, *col_perm = nullptr;
    double *l_val = nullptr, *u_val = nullptr;
    if ((rc = lu ? schwz_lu(n, sd->l_rp.data(), sd->l_col.data(), sd->l_val.data(), o.natural_factor_ordering, &l_rp,
                            &l_col, &l_val, &u_rp, &u_col, &u_val, &perm, &col_perm)
                 : schwz_cholesky(n, sd->l_rp.data(), sd->l_col.data(), sd->l_val.data(), o.natural_factor_ordering,
                                  &l_rp, &l_col, &l_val, &u_rp, &u_col, &u_val, &perm)))
        return rc;
    rc = lu ? schwz_trs_create_lu(n, l_rp, l_col, l_val, u_rp, u_col, u_val, perm, col_perm, &d->trs)
            : schwz_trs_create(n, l_rp, l_col, l_val, u_rp, u_col, u_val, perm, &d->trs);
    for (void *p : {(void *)l_rp, (void *)l_col, (void *)l_val, (void *)u_rp, (void *)u_col, (void *)u_val, (void *)perm,
                    (void *)col_perm})
        schwz_free(p);
    return rc;
}

// (the buffers, the pinned scalar and the event free themselves)
schwz_subdomain_device::~schwz_subdomain_device()
{
    delete batch;
    schwz_pcg_destroy(cg);
    schwz_pcg_f32_destroy(cg32);
    schwz_cheb_destroy(cheb);
    schwz_gmres_destroy(gmres);
    schwz_bicgstab_destroy(bicg);
    schwz_trs_destroy(trs);
    schwz_csr_destroy(A);
    delete coarse;
}

// the uploads of schwz_subdomain_to_device into the fresh sd->dev
static int upload_device_state(schwz_subdomain *sd, const double *h_local_rhs)
{
    schwz_subdomain_device *d = sd->dev;
    const int64_t n = sd->local_size_x;
    const int64_t nx = n + sd->halo_size;
    int rc;
    // every received id must have a slot in x~ and every interface column too
    std::vector<schwz_idx> put_idx, get_idx;
    put_idx.reserve((size_t)sd->num_send);
    get_idx.reserve((size_t)sd->num_recv);
    for (const auto &lst : sd->put)
        for (int64_t g : lst) put_idx.push_back((schwz_idx)(g - sd->first_row[sd->me]));
    for (const auto &lst : sd->get)
        for (int64_t g : lst) {
            const schwz_idx l = sd->to_local(g);
            SCHWZ_REQUIRE(l >= sd->local_size && l < nx, "get list id is not an overlap/halo id");
            get_idx.push_back(l);
        }
    // interface rows, compact over the overlap rows, columns -> x~ slots
    std::vector<schwz_idx> i_rp((size_t)sd->overlap_size + 1, 0), i_col(sd->i_col_global.size());
    for (int64_t r = 0; r < sd->overlap_size; ++r)
        i_rp[(size_t)r + 1] = sd->i_rp[(size_t)(sd->local_size + r) + 1];
    for (size_t k = 0; k < i_col.size(); ++k) {
        const schwz_idx l = sd->to_local(sd->i_col_global[k]);
        SCHWZ_REQUIRE(l >= n && l < nx, "interface column is not a halo id");
        i_col[k] = l;
    }
    sd->nnz_interface = (int64_t)i_col.size();
    if ((rc = schwz_csr_create(n, n, sd->l_rp.data(), sd->l_col.data(), sd->l_val.data(), &d->A))) return rc;
    // x~ and the CG iterate coincide on the interior: only tiles reaching the overlap need the
    // second product of the fused check+start residual kernel
    if (sd->overlap_size > 0 && (rc = csr_set_dual_split(d->A, sd->l_rp.data(), sd->l_col.data(), sd->local_size))) return rc;
    if ((rc = d->d_i_rp.put(i_rp)) || (rc = d->d_i_col.put(i_col)) || (rc = d->d_i_val.put(sd->i_val)) ||
        (rc = d->d_put_idx.put(put_idx)) || (rc = d->d_get_idx.put(get_idx)))
        return rc;
    if ((rc = d->d_x.alloc((size_t)(nx ? nx : 1), true))) return rc;  // (y: at the end, once the solver is known)
    if ((rc = d->d_rhs.put(h_local_rhs, (size_t)n)) || (rc = d->d_btilde.put(h_local_rhs, (size_t)n))) return rc;
    if ((rc = d->d_partials.alloc(2 * kMaxGrid + 2))) return rc;
    d->d_stream_part = stream_part_alloc(d->A->v);
    // (Pinned::alloc zeroes the scalars, which nothing relies on: a slot is written by a kernel before it is read)
    if ((rc = d->h_scalar.alloc(4, hipHostMallocMapped))) return rc;
    SCHWZ_HIP_TRY(hipHostGetDevicePointer((void **)&d->d_h_scalar, d->h_scalar.p, 0));
    if ((rc = d->ev_scalar.create())) return rc;
    if ((rc = create_local_solver(sd, put_idx))) return rc;
    // y: inside the x~ buffers where the two coincide (state A), else a vector of its own
    d->unified = want_unified(sd) && ensure_x_alt(sd);
    if (!d->unified && (rc = d->d_y.alloc((size_t)(n ? n : 1), true))) return rc;
    SCHWZ_HIP_TRY(hipDeviceSynchronize());
    return SCHWZ_OK;
}

extern "C" {

void schwz_subdomain_destroy(schwz_subdomain *sd)
{
    if (!sd) return;
    delete sd->dev;
    delete sd;
}

int schwz_subdomain_to_device(schwz_subdomain *sd, const double *h_local_rhs, const schwz_solver_options *opt)
{
    StageTimer timer_all("subdomain_to_device total");
    SCHWZ_REQUIRE(sd && h_local_rhs && opt, "schwz_subdomain_to_device: null argument");
    SCHWZ_REQUIRE(!sd->dev, "schwz_subdomain_to_device: already on the device");
    SCHWZ_REQUIRE(opt->local_solver == SCHWZ_SOLVER_ITERATIVE || opt->local_solver == SCHWZ_SOLVER_DIRECT ||
                      opt->local_solver == SCHWZ_SOLVER_DIRECT_LU,
                  "schwz_subdomain_to_device: unknown local solver");
    SCHWZ_REQUIRE(opt->par_ilu_sweeps >= 0 && opt->trisolve_sweeps >= 0,
                  "schwz_subdomain_to_device: par_ilu_sweeps / trisolve_sweeps must be >= 0");
    if ((opt->par_ilu_sweeps || opt->trisolve_sweeps) && opt->local_solver != SCHWZ_SOLVER_ITERATIVE) {
        set_error("schwz_subdomain_to_device: par_ilu_sweeps / trisolve_sweeps apply to the iterative local solver only");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    if (opt->local_solver == SCHWZ_SOLVER_ITERATIVE) {
        const int rc_sw = pcg_check_ilu_sweeps(opt->precond, opt->par_ilu_sweeps, opt->trisolve_sweeps);
        if (rc_sw) return rc_sw;
    }
    if (schwz_device_count() < 1) {
        set_error("schwz_subdomain_to_device: no HIP device visible (there is no CPU fallback)");
        return SCHWZ_ERR_HIP;
    }
    sd->opt = *opt;
    // a failure half way leaves nothing behind: the half-built device state is deleted here, not by a later destroy
    sd->dev = new schwz_subdomain_device();
    const int rc = upload_device_state(sd, h_local_rhs);
    if (rc) {
        delete sd->dev;
        sd->dev = nullptr;
    }
    return rc;
}

#define REQUIRE_DEVICE(sd, name) \
    SCHWZ_REQUIRE((sd) && (sd)->dev, name ": subdomain is not on the device")

int schwz_ras_pack(schwz_subdomain *sd, double *d_send, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_pack");
    if (sd->num_send == 0) return SCHWZ_OK;
    SCHWZ_REQUIRE(d_send, "schwz_ras_pack: null send buffer");
    return schwz_gather(sd->num_send, sd->dev->d_put_idx, sd->dev->d_x, d_send, SCHWZ_OP_COPY, stream);
}

int schwz_ras_unpack(schwz_subdomain *sd, const double *d_recv, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_unpack");
    if (sd->num_recv == 0) return SCHWZ_OK;
    SCHWZ_REQUIRE(d_recv, "schwz_ras_unpack: null recv buffer");
    return schwz_scatter(sd->num_recv, sd->dev->d_get_idx, d_recv, sd->dev->d_x, SCHWZ_OP_COPY, stream);
}

int schwz_ras_pack_f32(schwz_subdomain *sd, float *d_send, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_pack_f32");
    if (sd->num_send == 0) return SCHWZ_OK;
    SCHWZ_REQUIRE(d_send, "schwz_ras_pack_f32: null send buffer");
    return launch_gather_f32(sd->num_send, sd->dev->d_put_idx, sd->dev->d_x, d_send, (hipStream_t)stream);
}

int schwz_ras_unpack_f32(schwz_subdomain *sd, const float *d_recv, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_unpack_f32");
    if (sd->num_recv == 0) return SCHWZ_OK;
    SCHWZ_REQUIRE(d_recv, "schwz_ras_unpack_f32: null recv buffer");
    return launch_scatter_f32(sd->num_recv, sd->dev->d_get_idx, d_recv, sd->dev->d_x, (hipStream_t)stream);
}

// The pack of the NEXT exchange, beside the tail of the running local solve: waits (on `stream`, typically a
// side stream) for the event the solve records once the rows of the put lists are final, and gathers them
// from the solve's result y -- which the restriction copies to x~ unchanged, so the buffer holds what
// schwz_ras_pack would read after schwz_ras_restrict.
int schwz_ras_early_pack_ok(const schwz_subdomain *sd)
{
    return sd && sd->dev && local_kind(sd) == LocalKind::Cg && sd->dev->cg && sd->dev->cg->prio_on && sd->dev->cg->prio_event ? 1 : 0;
}

int schwz_ras_pack_early(schwz_subdomain *sd, void *d_send, int single, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_pack_early");
    SCHWZ_REQUIRE(schwz_ras_early_pack_ok(sd), "schwz_ras_pack_early: this subdomain's solver records no boundary event");
    if (sd->num_send == 0) return SCHWZ_OK;
    SCHWZ_REQUIRE(d_send, "schwz_ras_pack_early: null send buffer");
    SCHWZ_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, sd->dev->cg->prio_event, 0));
    if (single) return launch_gather_f32(sd->num_send, sd->dev->d_put_idx, y_of(sd), (float *)d_send, (hipStream_t)stream);
    return schwz_gather(sd->num_send, sd->dev->d_put_idx, y_of(sd), (double *)d_send, SCHWZ_OP_COPY, stream);
}

// One neighbour's part of the halo, to / from ANY device address -- the receiver's window in the
// free-running one-sided mode ("put": the pack kernel stores straight into the neighbour's receive
// buffer, mapped through schwz_ipc_open; "get": the unpack kernel loads from the neighbour's send buffer).
int schwz_ras_pack_neighbor(schwz_subdomain *sd, int k, void *d_dst, int single, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_pack_neighbor");
    SCHWZ_REQUIRE(k >= 0 && k < (int)sd->put.size(), "schwz_ras_pack_neighbor: no such out-neighbour");
    int64_t off = 0;
    for (int q = 0; q < k; ++q) off += (int64_t)sd->put[(size_t)q].size();
    const int64_t cnt = (int64_t)sd->put[(size_t)k].size();
    if (cnt == 0) return SCHWZ_OK;
    SCHWZ_REQUIRE(d_dst, "schwz_ras_pack_neighbor: null destination");
    if (single) return launch_gather_f32(cnt, sd->dev->d_put_idx + off, sd->dev->d_x, (float *)d_dst, (hipStream_t)stream);
    return schwz_gather(cnt, sd->dev->d_put_idx + off, sd->dev->d_x, (double *)d_dst, SCHWZ_OP_COPY, stream);
}

int schwz_ras_unpack_neighbor(schwz_subdomain *sd, int k, const void *d_src, int single, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_unpack_neighbor");
    SCHWZ_REQUIRE(k >= 0 && k < (int)sd->get.size(), "schwz_ras_unpack_neighbor: no such in-neighbour");
    int64_t off = 0;
    for (int q = 0; q < k; ++q) off += (int64_t)sd->get[(size_t)q].size();
    const int64_t cnt = (int64_t)sd->get[(size_t)k].size();
    if (cnt == 0) return SCHWZ_OK;
    SCHWZ_REQUIRE(d_src, "schwz_ras_unpack_neighbor: null source");
    if (single) return launch_scatter_f32(cnt, sd->dev->d_get_idx + off, (const float *)d_src, sd->dev->d_x, (hipStream_t)stream);
    return schwz_scatter(cnt, sd->dev->d_get_idx + off, (const double *)d_src, sd->dev->d_x, SCHWZ_OP_COPY, stream);
}

// ---- windows: device buffers other rank processes map (the MPI_Win_create of communicate.hpp:67-224) ----

int schwz_window_alloc(int64_t bytes, void **d_ptr)
{
    SCHWZ_REQUIRE(d_ptr && bytes >= 0, "schwz_window_alloc: bad arguments");
    *d_ptr = nullptr;
    // an allocation of its own (not a piece of a pooled one): the IPC handle names exactly this buffer
    SCHWZ_HIP_TRY(hipMalloc(d_ptr, (size_t)(bytes > 0 ? bytes : 16)));
    SCHWZ_HIP_TRY(hipMemset(*d_ptr, 0, (size_t)(bytes > 0 ? bytes : 16)));
    return SCHWZ_OK;
}

int schwz_window_free(void *d_ptr)
{
    if (d_ptr) SCHWZ_HIP_TRY(hipFree(d_ptr));
    return SCHWZ_OK;
}

int schwz_window_export(void *d_ptr, unsigned char *h_handle64)
{
    SCHWZ_REQUIRE(d_ptr && h_handle64, "schwz_window_export: null argument");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    hipIpcMemHandle_t h;
    SCHWZ_HIP_TRY(hipIpcGetMemHandle(&h, d_ptr));
    std::memcpy(h_handle64, &h, 64);
    return SCHWZ_OK;
}

int schwz_window_open(const unsigned char *h_handle64, void **d_ptr)
{
    SCHWZ_REQUIRE(d_ptr && h_handle64, "schwz_window_open: null argument");
    hipIpcMemHandle_t h;
    std::memcpy(&h, h_handle64, 64);
    *d_ptr = nullptr;
    SCHWZ_HIP_TRY(hipIpcOpenMemHandle(d_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return SCHWZ_OK;
}

int schwz_window_close(void *d_ptr)
{
    if (d_ptr) SCHWZ_HIP_TRY(hipIpcCloseMemHandle(d_ptr));
    return SCHWZ_OK;
}

int schwz_ras_update_boundary(schwz_subdomain *sd, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_update_boundary");
    // rows < local_size have no interface entries: b~ = b there, set at upload.
    // restricted_schwarz.cpp:1007: only applied when num_subdomains > 1 && overlap > 0
    if (sd->P <= 1 || sd->nnz_interface == 0) return SCHWZ_OK;
    return launch_interface_update(sd->overlap_size, sd->local_size, sd->dev->d_i_rp, sd->dev->d_i_col, sd->dev->d_i_val,
                                   sd->dev->d_x, sd->dev->d_rhs, sd->dev->d_btilde, (hipStream_t)stream);
}

// Launches the residual-norm kernels and the 8-byte device->host copy, then records
// an event: the host can wait for the scalar alone while later launches (the local
// solve) already run behind it on the same stream.
static int residual_norm_sq_launch(schwz_subdomain *sd, const double *b, int64_t row_limit, hipStream_t st)
{
    schwz_subdomain_device *d = sd->dev;
    SpmvArgs a;
    a.x = d->d_x;
    a.b = b;
    a.partials = d->d_partials;
    a.stream_part = d->d_stream_part;
    a.row_limit = row_limit;
    int rc = launch_spmv(d->A->v, kSpmvResidNorm, a, sd->opt.spmv_variant, st);
    if (rc) return rc;
    const int g = spmv_grid(d->A->v, sd->opt.spmv_variant);
    // the scalar lands in mapped pinned host memory straight from the kernel: no
    // copy engine hop between this kernel and the next one in the stream
    if ((rc = launch_final_norm(d->d_partials + g, g, d->d_h_scalar, st))) return rc;
    SCHWZ_HIP_TRY(hipEventRecord(d->ev_scalar, st));
    return SCHWZ_OK;
}

int schwz_ras_local_residual_launch(schwz_subdomain *sd, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_local_residual_launch");
    if (sd->local_size_x == 0) return SCHWZ_OK;
    return residual_norm_sq_launch(sd, sd->dev->d_btilde, sd->local_size_x, (hipStream_t)stream);
}

int schwz_ras_local_residual_wait(schwz_subdomain *sd, double *h_resnorm)
{
    REQUIRE_DEVICE(sd, "schwz_ras_local_residual_wait");
    SCHWZ_REQUIRE(h_resnorm, "schwz_ras_local_residual_wait: null output");
    if (sd->local_size_x == 0) {
        *h_resnorm = 0.0;
        return SCHWZ_OK;
    }
    SCHWZ_HIP_TRY(hipEventSynchronize(sd->dev->ev_scalar));
    *h_resnorm = std::sqrt(sd->dev->h_scalar.p[0]);
    if (*h_resnorm != *h_resnorm) {
        // a NaN norm: say so specifically when it comes from a triangular sweep that gave up waiting
        int rc = sd->dev->cg ? pcg_take_trs_error(sd->dev->cg) : SCHWZ_OK;
        if (!rc && sd->dev->trs) rc = trs_take_error(sd->dev->trs);
        if (rc) return rc;
    }
    return SCHWZ_OK;
}

namespace schwz {
__global__ void copy_scalar_kernel(const double *src, double *dst)
{
    dst[0] = src[0];  // src: mapped pinned host memory, final once the norm's event has fired
}
}  // namespace schwz

int schwz_ras_norm_sq_to_device(schwz_subdomain *sd, double *d_norm_sq, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_norm_sq_to_device");
    SCHWZ_REQUIRE(d_norm_sq, "schwz_ras_norm_sq_to_device: null output");
    hipStream_t st = (hipStream_t)stream;
    if (sd->local_size_x == 0) {
        SCHWZ_HIP_TRY(hipMemsetAsync(d_norm_sq, 0, sizeof(double), st));
        return SCHWZ_OK;
    }
    SCHWZ_HIP_TRY(hipStreamWaitEvent(st, sd->dev->ev_scalar, 0));
    hipLaunchKernelGGL(schwz::copy_scalar_kernel, dim3(1), dim3(1), 0, st, (const double *)sd->dev->d_h_scalar, d_norm_sq);
    SCHWZ_HIP_TRY(hipGetLastError());
    return SCHWZ_OK;
}

int schwz_ras_local_residual(schwz_subdomain *sd, double *h_resnorm, schwz_stream stream)
{
    int rc = schwz_ras_local_residual_launch(sd, stream);
    if (rc) return rc;
    return schwz_ras_local_residual_wait(sd, h_resnorm);
}

int schwz_ras_true_residual_sq(schwz_subdomain *sd, double *h_out, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_true_residual_sq");
    SCHWZ_REQUIRE(h_out, "schwz_ras_true_residual_sq: null output");
    if (sd->local_size == 0) {
        *h_out = 0.0;
        return SCHWZ_OK;
    }
    int rc = residual_norm_sq_launch(sd, sd->dev->d_rhs, sd->local_size, (hipStream_t)stream);
    if (rc) return rc;
    SCHWZ_HIP_TRY(hipEventSynchronize(sd->dev->ev_scalar));
    *h_out = sd->dev->h_scalar.p[0];
    return SCHWZ_OK;
}

// (A x~) on the interior rows, kept (the outer FGMRES, csrc/outer.hip): the local matrix in the coding the residual
// launches read, over all its local_size_x rows.  Without overlap rows the pass writes d_out itself; otherwise it goes
// through d_apply, whose first local_size entries are copied.
int schwz_ras_apply_interior(schwz_subdomain *sd, double *d_out, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_apply_interior");
    SCHWZ_REQUIRE(d_out || sd->local_size == 0, "schwz_ras_apply_interior: null output");
    if (sd->local_size == 0) return SCHWZ_OK;
    schwz_subdomain_device *d = sd->dev;
    hipStream_t st = (hipStream_t)stream;
    const bool direct = sd->local_size_x == sd->local_size && ((uintptr_t)d_out & 15u) == 0;
    int rc;
    if (!direct && !d->d_apply && (rc = d->d_apply.alloc((size_t)sd->local_size_x, true))) return rc;
    SpmvArgs a;
    a.x = d->d_x;
    a.y = direct ? d_out : (double *)d->d_apply;
    a.stream_part = d->d_stream_part;
    if ((rc = launch_spmv(d->A->v, kSpmvPlain, a, sd->opt.spmv_variant, st))) return rc;
    return direct ? SCHWZ_OK : launch_copy_any(sd->local_size, d->d_apply, d_out, st);
}

int schwz_ras_set_local_max_iters(schwz_subdomain *sd, int max_iters)
{
    SCHWZ_REQUIRE(sd && sd->dev, "schwz_ras_set_local_max_iters: subdomain is not on the device");
    SCHWZ_REQUIRE(max_iters >= -1, "schwz_ras_set_local_max_iters: max_iters must be -1 or >= 0");
    sd->opt.local_max_iters = max_iters;
    return SCHWZ_OK;
}

int schwz_ras_last_inner_stats(schwz_subdomain *sd, int *h_iters, double *h_resnorm)
{
    REQUIRE_DEVICE(sd, "schwz_ras_last_inner_stats");
    schwz_subdomain_device *d = sd->dev;
    SCHWZ_REQUIRE(h_iters && h_resnorm, "schwz_ras_last_inner_stats: null output");
    *h_iters = 0;
    *h_resnorm = 0.0;
    if (sd->local_size_x == 0) return SCHWZ_OK;
    switch (local_kind(sd)) {
    case LocalKind::Direct: return SCHWZ_OK;
    case LocalKind::Gmres: return schwz_gmres_last_stats(d->gmres, h_iters, h_resnorm);
    case LocalKind::Bicgstab: return schwz_bicgstab_last_stats(d->bicg, h_iters, h_resnorm);
    case LocalKind::CgF32: return schwz_pcg_f32_last_stats(d->cg32, h_iters, h_resnorm);
    case LocalKind::Chebyshev: return schwz_cheb_last_stats(d->cheb, h_iters, h_resnorm);
    case LocalKind::Cg: return d->cg ? pcg_last_stats(d->cg, h_iters, h_resnorm) : SCHWZ_OK;
    }
    return SCHWZ_OK;
}

int schwz_ras_local_solve(schwz_subdomain *sd, int *h_inner_iters, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_local_solve");
    if (local_kind(sd) != LocalKind::Cg) return solve_in_place(sd, h_inner_iters, stream);
    SCHWZ_REQUIRE(sd->dev->cg, "schwz_ras_local_solve: the subdomain has no iterative solver");
    const int rc = choose_form(sd, (hipStream_t)stream);
    if (rc) return rc;
    return cg_solve_in_form(sd, [&](double *y) {
        return schwz_pcg_solve(sd->dev->cg, sd->dev->d_btilde, y, sd->opt.local_tol, local_maxit(sd), h_inner_iters, nullptr, stream);
    });
}

int schwz_ras_check_and_solve_launch(schwz_subdomain *sd, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_check_and_solve_launch");
    schwz_subdomain_device *d = sd->dev;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = sd->local_size_x;
    if (n == 0) return SCHWZ_OK;
    // the check residual shares the matrix pass of the CG start residual (kSpmvResidDual) ...
    if (local_kind(sd) == LocalKind::Cg && d->cg && spmv_variant_has_dual(sd->opt.spmv_variant)) {
        int rc = choose_form(sd, st);
        if (rc) return rc;
        // x~ and y coincide on [interior|overlap] when there is no overlap at all
        // (single subdomain): the check residual is then the CG start residual ...
        const double *x2 = (sd->overlap_size == 0) ? nullptr : d->d_x;
        // ... unless a solve has run since the last restriction (a discarded solve, x~ kept): y has moved on and the
        // check residual, which belongs to x~, gets its own launch
        if (x2 || !(d->unified ? d->y_in_alt : d->y_ahead))
            return cg_solve_in_form(sd, [&](double *y) {
                schwz_pcg *cg = d->cg;
                double *keep = cg->d_norm_sq;
                cg->d_norm_sq = d->d_h_scalar;  // mapped pinned host memory, written by the kernel
                int rc = pcg_begin(cg, d->d_btilde, y, sd->opt.local_tol, true, x2, n, st);
                cg->d_norm_sq = keep;
                if (!rc) {
                    // the norm is final behind the start launch's fold: a kernel of pcg_begin, or the first launch of
                    // pcg_iterate, which then records the event (nothing on the device waits for it earlier:
                    // schwz_ras_norm_sq_to_device is enqueued after this function)
                    if (cg->init.pending)
                        cg->init_event = d->ev_scalar;
                    else if (hipEventRecord(d->ev_scalar, st) != hipSuccess)
                        rc = SCHWZ_ERR_HIP;
                }
                if (!rc) rc = pcg_iterate(cg, y, sd->opt.local_tol, local_maxit(sd), st);
                cg->init_event = nullptr;
                return rc;
            });
    }
    // ... where a kernel for it exists; otherwise the two steps back to back
    const int rc = schwz_ras_local_residual_launch(sd, stream);
    if (rc) return rc;
    return schwz_ras_local_solve(sd, nullptr, stream);
}

int schwz_ras_restrict(schwz_subdomain *sd, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_restrict");
    schwz_subdomain_device *d = sd->dev;
    if (sd->local_size == 0) return SCHWZ_OK;
    if (d->unified) {
        // state B: the buffer the solve filled becomes x~ (and y stays where it is: state A).  State A: y is x~.
        if (d->y_in_alt) std::swap(d->d_x, d->d_x_alt);
        d->y_in_alt = false;
        return SCHWZ_OK;
    }
    d->y_ahead = false;
    if (d->cg && d->cg->x2_written && d->d_x_alt && d->cg->x2_out == d->d_x_alt) {
        // the solve's last x update wrote y[interior] into the other buffer: it becomes x~
        std::swap(d->d_x, d->d_x_alt);
        d->cg->x2_written = false;
        d->cg->x2_out = d->d_x_alt;
        return SCHWZ_OK;
    }
    return launch_copy(sd->local_size, d->d_y, d->d_x, (hipStream_t)stream);
}

// Between two solves on a set-up subdomain (an extension; the right-hand side itself is replaced by the calls of
// rhs.hip).  First the solver objects forget their last solve -- a postponed launch is dropped BEFORE any buffer is
// rewritten, never run later on the new data.  keep_x = 0 then leaves what schwz_subdomain_to_device leaves: the form
// the upload would choose for the solver that is selected now (a setter that changed the kind has already moved y to
// a vector of its own, as it does behind a fresh upload), y where that form keeps it, and one pass over the vectors.
// keep_x = 1 keeps every vector and both form flags -- a y that is ahead of x~ stays ahead -- and only copies b to
// b~: its interior rows are written nowhere else (schwz_ras_update_boundary rewrites the overlap rows alone).
int schwz_ras_restart(schwz_subdomain *sd, int keep_x, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_restart");
    schwz_subdomain_device *d = sd->dev;
    SCHWZ_REQUIRE(keep_x == 0 || keep_x == 1, "schwz_ras_restart: keep_x must be 0 or 1");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = pcg_forget(d->cg, st)) || (rc = pcg_f32_forget(d->cg32, st)) || (rc = cheb_forget(d->cheb, st)) ||
        (rc = gmres_forget(d->gmres, st)) || (rc = bicgstab_forget(d->bicg, st)))
        return rc;
    const int64_t n = sd->local_size_x;
    if (keep_x) return launch_copy(n, d->d_rhs, d->d_btilde, st);
    const bool uni = want_unified(sd) && ensure_x_alt(sd);
    // (the pass below zeroes it: no memset of its own)
    if (!uni && !d->d_y && (rc = d->d_y.alloc((size_t)(n ? n : 1)))) return rc;
    d->unified = uni;
    d->y_in_alt = false;
    d->y_ahead = false;
    return launch_restart(n, n + sd->halo_size, d->d_rhs, d->d_btilde, d->d_x, d->d_x_alt, d->d_y, st);
}

// The coarse correction c (schwz_coarse_solve) added to every copy of every row this subdomain holds: all slots of
// x~, and the warm start y of the next local solve on its local_size_x entries -- a short inner solve would otherwise
// undo the correction.  Where y lives is y_of's answer at this moment: a buffer of its own (d_y; or, unified state B,
// the other x~ buffer) takes the same launch, and where y IS x~ (unified state A) the one pass adds once.  Nothing
// here changes the form: the next solve's choose_form copies a corrected y, its x2_out pass copies the corrected
// overlap / halo entries of d_x, and the postponed residual update of a lazy last iteration reads neither vector.
int schwz_ras_coarse_apply(schwz_subdomain *sd, schwz_coarse *c, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_coarse_apply");
    schwz_subdomain_device *d = sd->dev;
    SCHWZ_REQUIRE(d->coarse, "schwz_ras_coarse_apply: the subdomain has no aggregates (schwz_ras_coarse_set_aggregates)");
    SCHWZ_REQUIRE(c, "schwz_ras_coarse_apply: null coarse object");
    double *y = y_of(sd);
    if (y == d->d_x) y = nullptr;
    return launch_coarse_apply(d->coarse, c, d->d_x, sd->local_size_x + sd->halo_size, y, y ? sd->local_size_x : 0,
                               (hipStream_t)stream);
}

int schwz_ras_vector(schwz_subdomain *sd, int which, double **d_ptr, int64_t *len)
{
    REQUIRE_DEVICE(sd, "schwz_ras_vector");
    SCHWZ_REQUIRE(d_ptr && len, "schwz_ras_vector: null output");
    switch (which) {
    case 0: *d_ptr = sd->dev->d_x; *len = sd->local_size_x + sd->halo_size; break;
    case 1: *d_ptr = sd->dev->d_btilde; *len = sd->local_size_x; break;
    case 2: *d_ptr = y_of(sd); *len = sd->local_size_x; break;
    case 3: *d_ptr = sd->dev->d_rhs; *len = sd->local_size_x; break;
    default: set_error("schwz_ras_vector: unknown vector id"); return SCHWZ_ERR_INVALID;
    }
    return SCHWZ_OK;
}

int schwz_ras_local_csr(schwz_subdomain *sd, schwz_csr **out)
{
    REQUIRE_DEVICE(sd, "schwz_ras_local_csr");
    SCHWZ_REQUIRE(out, "schwz_ras_local_csr: null output");
    *out = sd->dev->A;
    return SCHWZ_OK;
}

// 0 none, 1 full 1/diag vector, 2 one-byte codes into a dictionary, 3 one scalar (schwz::DiagView)
int schwz_ras_jacobi_form(const schwz_subdomain *sd) { return sd && sd->dev && sd->dev->cg ? sd->dev->cg->diag.mode : 0; }

int schwz_ras_y_form(const schwz_subdomain *sd) { return sd && sd->dev && sd->dev->unified ? (sd->dev->y_in_alt ? 2 : 1) : 0; }

int schwz_ras_cg_flavour(const schwz_subdomain *sd)
{
    return sd && sd->dev && local_kind(sd) == LocalKind::Cg && sd->dev->cg ? schwz_pcg_flavour(sd->dev->cg) : 0;
}

int schwz_ras_local_precision(const schwz_subdomain *sd) { return sd ? sd->precision : SCHWZ_PRECISION_F64; }

// The fp32 CG and the Chebyshev solver stand in for the CG of a symmetric matrix without a preconditioner or with
// scalar Jacobi: SCHWZ_PRECOND_NONE or SCHWZ_PRECOND_JACOBI, whichever they are to be created with; -1: not such a
// subdomain.
static int plain_cg_precond(const schwz_subdomain *sd)
{
    const schwz_solver_options &o = sd->opt;
    if (o.local_solver != SCHWZ_SOLVER_ITERATIVE || o.non_symmetric || !sd->dev->cg) return -1;
    if (o.precond == SCHWZ_PRECOND_NONE) return SCHWZ_PRECOND_NONE;
    if (o.precond == SCHWZ_PRECOND_JACOBI || (o.precond == SCHWZ_PRECOND_BLOCK_JACOBI && o.precond_block_size <= 1))
        return SCHWZ_PRECOND_JACOBI;
    return -1;
}

// behind a setter that changed local_kind: y moves to where the new kind keeps it (a vector of its own:
// schwz_ras_y_form answers 0 from here on)
static int settle_form(schwz_subdomain *sd)
{
    // a solve still in flight on a stream the null stream does not wait for must not race with the copy below
    SCHWZ_HIP_TRY(hipDeviceSynchronize());
    const int rc = choose_form(sd, nullptr);
    if (rc) return rc;
    SCHWZ_HIP_TRY(hipDeviceSynchronize());
    return SCHWZ_OK;
}

int schwz_ras_set_local_precision(schwz_subdomain *sd, int precision)
{
    REQUIRE_DEVICE(sd, "schwz_ras_set_local_precision");
    SCHWZ_REQUIRE(precision == SCHWZ_PRECISION_F64 || precision == SCHWZ_PRECISION_F32,
                  "schwz_ras_set_local_precision: unknown precision");
    if (precision == SCHWZ_PRECISION_F64) {
        sd->precision = precision;  // (the next solve chooses its form again: choose_form)
        return SCHWZ_OK;
    }
    const int precond = plain_cg_precond(sd);
    if (precond < 0) {
        set_error("schwz_ras_set_local_precision: the fp32 local solve exists for the iterative solver of a symmetric "
                  "matrix (CG) without a preconditioner or with scalar Jacobi only");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    if (sd->sym_solver == SCHWZ_SYM_CHEBYSHEV) {
        set_error("schwz_ras_set_local_precision: the Chebyshev local solve has no fp32 form");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    int rc;
    if (!sd->dev->cg32 && (rc = schwz_pcg_f32_create(sd->dev->A, precond, &sd->dev->cg32))) return rc;
    sd->precision = precision;
    return settle_form(sd);
}

int schwz_ras_sym_solver(const schwz_subdomain *sd) { return sd ? sd->sym_solver : SCHWZ_SYM_CG; }

int schwz_ras_set_sym_solver(schwz_subdomain *sd, int which)
{
    SCHWZ_REQUIRE(sd, "schwz_ras_set_sym_solver: null subdomain");
    SCHWZ_REQUIRE(which == SCHWZ_SYM_CG || which == SCHWZ_SYM_CHEBYSHEV, "schwz_ras_set_sym_solver: unknown solver");
    REQUIRE_DEVICE(sd, "schwz_ras_set_sym_solver");
    if (which == SCHWZ_SYM_CG) {
        sd->sym_solver = which;  // (the next solve chooses its form again: choose_form)
        return SCHWZ_OK;
    }
    const int precond = plain_cg_precond(sd);
    if (precond < 0 || sd->opt.par_ilu_sweeps != 0 || sd->opt.trisolve_sweeps != 0) {
        set_error("schwz_ras_set_sym_solver: the Chebyshev local solve exists for the iterative solver of a symmetric "
                  "matrix without a preconditioner or with scalar Jacobi only (no ParILU options)");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    if (sd->precision == SCHWZ_PRECISION_F32) {
        set_error("schwz_ras_set_sym_solver: the Chebyshev local solve has no fp32 form (SCHWZ_PRECISION_F32 is set)");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    int rc;
    if (!sd->dev->cheb && (rc = schwz_cheb_create(sd->dev->A, precond, &sd->dev->cheb))) return rc;
    sd->sym_solver = which;
    return settle_form(sd);
}

int schwz_ras_cheb_bounds(const schwz_subdomain *sd, double *lmin, double *lmax)
{
    SCHWZ_REQUIRE(sd && sd->dev && sd->dev->cheb, "schwz_ras_cheb_bounds: the subdomain has no Chebyshev solver (schwz_ras_set_sym_solver)");
    return schwz_cheb_bounds(sd->dev->cheb, lmin, lmax);
}

int schwz_ras_set_cheb_bounds(schwz_subdomain *sd, double lmin, double lmax)
{
    SCHWZ_REQUIRE(sd && sd->dev && sd->dev->cheb, "schwz_ras_set_cheb_bounds: the subdomain has no Chebyshev solver (schwz_ras_set_sym_solver)");
    return schwz_cheb_set_bounds(sd->dev->cheb, lmin, lmax);
}

int schwz_ras_nonsym_solver(const schwz_subdomain *sd) { return sd && sd->dev && sd->dev->bicg ? SCHWZ_NONSYM_BICGSTAB : SCHWZ_NONSYM_GMRES; }

int schwz_ras_set_nonsym_solver(schwz_subdomain *sd, int which)
{
    SCHWZ_REQUIRE(sd, "schwz_ras_set_nonsym_solver: null subdomain");
    SCHWZ_REQUIRE(which == SCHWZ_NONSYM_GMRES || which == SCHWZ_NONSYM_BICGSTAB,
                  "schwz_ras_set_nonsym_solver: unknown solver");
    REQUIRE_DEVICE(sd, "schwz_ras_set_nonsym_solver");
    schwz_subdomain_device *d = sd->dev;
    // (exactly one of gmres / bicg and no cg: what local_kind relies on)
    if (sd->opt.local_solver != SCHWZ_SOLVER_ITERATIVE || !sd->opt.non_symmetric || !d->gmres == !d->bicg || d->cg) {
        set_error("schwz_ras_set_nonsym_solver: the choice exists for the iterative local solver of a non-symmetric "
                  "matrix only");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    if (which == schwz_ras_nonsym_solver(sd)) return SCHWZ_OK;
    // a solve still in flight must not lose its work vectors
    SCHWZ_HIP_TRY(hipDeviceSynchronize());
    // The preconditioner object (Jacobi diagonal, block inverses, ILU / ISAI factors, its partial-sum banks) is
    // handed over: neither solver keeps state of a solve in it.  The new solver is created around it first, while
    // the old one still owns it; a failure (no memory for the work vectors) leaves the subdomain as it was.
    int rc;
    if (which == SCHWZ_NONSYM_BICGSTAB) {
        if ((rc = bicgstab_create_adopt(d->A, gmres_precond(d->gmres), &d->bicg))) return rc;
        (void)gmres_release_precond(d->gmres);
        schwz_gmres_destroy(d->gmres);
        d->gmres = nullptr;
        return SCHWZ_OK;
    }
    if ((rc = gmres_create_adopt(d->A, sd->opt.restart_iter < 1 ? 1 : sd->opt.restart_iter, sd->gmres_basis,
                                 bicgstab_precond(d->bicg), &d->gmres)))
        return rc;
    (void)bicgstab_release_precond(d->bicg);
    schwz_bicgstab_destroy(d->bicg);
    d->bicg = nullptr;
    return SCHWZ_OK;
}

int schwz_ras_gmres_basis(const schwz_subdomain *sd) { return sd ? sd->gmres_basis : SCHWZ_GMRES_BASIS_F64; }

int schwz_ras_set_gmres_basis(schwz_subdomain *sd, int which)
{
    SCHWZ_REQUIRE(sd, "schwz_ras_set_gmres_basis: null subdomain");
    SCHWZ_REQUIRE(which == SCHWZ_GMRES_BASIS_F64 || which == SCHWZ_GMRES_BASIS_F32,
                  "schwz_ras_set_gmres_basis: unknown basis type");
    REQUIRE_DEVICE(sd, "schwz_ras_set_gmres_basis");
    schwz_subdomain_device *d = sd->dev;
    if (sd->opt.local_solver != SCHWZ_SOLVER_ITERATIVE || !sd->opt.non_symmetric || !d->gmres == !d->bicg || d->cg) {
        set_error("schwz_ras_set_gmres_basis: the choice exists for the iterative local solver of a non-symmetric "
                  "matrix only");
        return SCHWZ_ERR_NOT_IMPLEMENTED;
    }
    if (which == sd->gmres_basis) return SCHWZ_OK;
    if (d->gmres) {
        // as in schwz_ras_set_nonsym_solver: the new solver is created around the preconditioner while the old one
        // still owns it, so a failure leaves the subdomain as it was
        SCHWZ_HIP_TRY(hipDeviceSynchronize());
        schwz_gmres *fresh = nullptr;
        const int rc = gmres_create_adopt(d->A, sd->opt.restart_iter < 1 ? 1 : sd->opt.restart_iter, which,
                                          gmres_precond(d->gmres), &fresh);
        if (rc) return rc;
        (void)gmres_release_precond(d->gmres);
        schwz_gmres_destroy(d->gmres);
        d->gmres = fresh;
    }
    sd->gmres_basis = which;  // (while BiCGSTAB is set: what a return to GMRES creates)
    return SCHWZ_OK;
}

int schwz_ras_get_interior(schwz_subdomain *sd, double *h_out, schwz_stream stream)
{
    REQUIRE_DEVICE(sd, "schwz_ras_get_interior");
    SCHWZ_REQUIRE(h_out || sd->local_size == 0, "schwz_ras_get_interior: null output");
    if (sd->local_size == 0) return SCHWZ_OK;
    SCHWZ_HIP_TRY(hipMemcpyAsync(h_out, sd->dev->d_x, (size_t)sd->local_size * sizeof(double), hipMemcpyDeviceToHost,
                                 (hipStream_t)stream));
    SCHWZ_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return SCHWZ_OK;
}

// B_spmv = 12 nnz + 4 (n+1) + 16 n ; one PCG iteration = B_spmv + 136 n
int64_t schwz_ras_algorithmic_bytes(const schwz_subdomain *sd, int which)
{
    if (!sd) return 0;
    const int64_t n = sd->local_size_x, nnz = (int64_t)sd->l_col.size();
    const int64_t spmv = 12 * nnz + 4 * (n + 1) + 16 * n;
    if (which == 0) return spmv;
    if (which == 2) {
        // the coarse step of this subdomain (coarse.hip): W (value, slot, gathered x~) and the aggregates' beta and s;
        // its m rows of the GEMV over the explicit inverse with s read and c written; the apply pass -- x~ read and
        // written and two bytes of id per slot, and y read and written where it is a buffer of its own
        const schwz_coarse_part *p = sd->dev ? sd->dev->coarse : nullptr;
        if (!p) return 0;
        const int64_t slots = p->nslots;
        const bool own_y = !(sd->dev->unified && !sd->dev->y_in_alt);
        return 20 * p->nw + 16 * (int64_t)p->m + 8 * (int64_t)p->m * p->nc + 16 * (int64_t)p->nc + 16 * slots + 2 * slots +
               (own_y ? 16 * n : 0);
    }
    if (which == 3) {
        // schwz_ras_aggregate_sums (coarse.hip): a value and a row id per interior row; per piece its record, and its
        // partial sum stored and read; the offsets of the fold and the m sums stored
        const schwz_coarse_part *p = sd->dev ? sd->dev->coarse : nullptr;
        if (!p) return 0;
        return 12 * sd->local_size + 28 * (int64_t)p->nrow_pieces + 4 * ((int64_t)p->m + 1) + 8 * (int64_t)p->m;
    }
    switch (local_kind(sd)) {
    case LocalKind::CgF32:
        // cg_f32.hip: 8 B per nonzero, p gathered and q stored in fp32, then e, r read and written, p, q, 1/diag read
        // (update launch) and p read and written, r, 1/diag read (direction launch): 44 B per row
        return 8 * nnz + 4 * (n + 1) + 8 * n + 44 * n;
    case LocalKind::Chebyshev:
        // the fused launch of chebyshev.hip: the CSR stream, then per row d read and d' written, r and x read and
        // written, 1/diag read with Jacobi
        return 12 * nnz + 4 * (n + 1) + (sd->opt.precond == SCHWZ_PRECOND_NONE ? 48 : 56) * n;
    default: return spmv + 136 * n;
    }
}

}  // extern "C"
