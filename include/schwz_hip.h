/*
 * schwz_hip.h -- C ABI of libschwz_hip.so, the MI355X (gfx950) implementation of
 * the Restricted Additive Schwarz hot path of pratikvn/schwarz-lib.
 *
 * Every entry point names the reference interface it replaces (paths relative
 * to the reference checkout).  The reference itself is a C++ template library
 * over Ginkgo types (no FFI); this header is the boundary a host layer binds:
 * the C++ mirror of SolverRAS/SchwarzBase (schwarz-lib_amd/host/), the Python
 * host used by bench.py/tests (schwarz-lib_amd/schwz_amd/), or the binding
 * sketched in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / Ginkgo types.
 *   - `d_` pointers are device (HBM) pointers, `h_` pointers are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *     All device entry points are asynchronous on `stream` unless noted.
 *     Any stream will do, blocking or not: every launch, copy and event of a
 *     call goes to the stream it was handed (graphs are captured on a private
 *     stream and replayed on the caller's), and nothing is left to the default
 *     stream.  Calls that hand a value back to the host (h_iters / h_resnorm,
 *     the *_wait, *_last_stats, get_interior and true_residual_sq calls) wait
 *     for it; a solve with rtol > 0 polls its state, and GMRES / BiCGSTAB look
 *     at theirs once per cycle / per SCHWZ_BICGSTAB_POLL_BATCH iterations.
 *   - creation calls (schwz_*_create*, schwz_subdomain_to_device,
 *     schwz_window_alloc) take no stream and are complete on return: the
 *     object may be used on any stream at once.
 *   - one object (solver, triangular solve, subdomain) is used on one stream at
 *     a time; the caller orders a change of stream with an event.  Exceptions
 *     are the calls documented to run beside a solve on a second stream
 *     (schwz_ras_pack_early, schwz_ras_norm_sq_to_device).
 *   - a matrix (schwz_csr) is read-only once created: any number of solvers and
 *     subdomains created on one matrix may run at the same time on different
 *     streams.  Destroy a matrix after the objects created on it.
 *   - values are fp64 (bench_ras.cpp:204 fixes BenchRas<double,int>), local
 *     indices int32, global row ids int64 (1024^3 rows fit int32, global nnz
 *     does not -- SURVEY F7).
 *   - return value: SCHWZ_OK or an error code; schwz_last_error() holds the
 *     message (the reference throws the Error hierarchy of
 *     include/exception.hpp:42-210; the host mirrors re-throw from the code).
 *   - there is NO CPU fallback: device entry points fail with SCHWZ_ERR_HIP
 *     when no GPU is present.
 */
#ifndef SCHWZ_HIP_H
#define SCHWZ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t schwz_idx;
typedef void *schwz_stream;

enum schwz_status {
    SCHWZ_OK = 0,
    SCHWZ_ERR_INVALID = 1,         /* BadDimension / bad argument */
    SCHWZ_ERR_HIP = 2,             /* CudaError equivalent (exception.hpp:133-152) */
    SCHWZ_ERR_NOT_IMPLEMENTED = 3, /* NotImplemented (exception.hpp:81-96) */
    SCHWZ_ERR_NOT_SPD = 4,         /* factorization failed */
    SCHWZ_ERR_IO = 5,              /* matrix file missing (initialization.cpp:266-271) */
    SCHWZ_ERR_DIVERGED = 6         /* NaN / >1e12 residual (schwarz_base.cpp:424-428) */
};

/* include/collective_common.hpp:36 */
enum schwz_op { SCHWZ_OP_ADD = 0, SCHWZ_OP_COPY = 1, SCHWZ_OP_DIFF = 2, SCHWZ_OP_AVG = 3 };

/* Settings::local_solver_settings (include/settings.hpp) as used by
 * Solve::local_solve (source/solve.cpp:667-792) */
/* SCHWZ_SOLVER_DIRECT: LL^T (schwz_cholesky, "cholmod"); SCHWZ_SOLVER_DIRECT_LU: pivoted LU
 * (schwz_lu, settings.factorization == "umfpack"), also for non-symmetric matrices.  Both run
 * the triangular solves on the GPU (schwz_trs). */
enum schwz_local_solver { SCHWZ_SOLVER_ITERATIVE = 0, SCHWZ_SOLVER_DIRECT = 1, SCHWZ_SOLVER_DIRECT_LU = 2 };
/* metadata.local_precond (source/solve.cpp:486-652): "null", "block-jacobi"
 * (gko::preconditioner::Jacobi, :490-505,575-589) and "ilu" (ParIlu + LowerTrs/UpperTrs,
 * :506-532,590-615) and "isai" (Ilu<LowerIsai, UpperIsai>, :616-638) */
enum schwz_precond {
    SCHWZ_PRECOND_NONE = 0,
    SCHWZ_PRECOND_JACOBI = 1,       /* block-jacobi, precond_max_block_size = 1 */
    SCHWZ_PRECOND_BLOCK_JACOBI = 2, /* block-jacobi, consecutive blocks of precond_max_block_size rows */
    SCHWZ_PRECOND_ILU = 3,          /* ilu: ILU(0) + lower/upper triangular sweeps per iteration */
    SCHWZ_PRECOND_ISAI = 4          /* isai: ILU(0) factors replaced by their ISAIs, two SpMVs per application */
};

const char *schwz_last_error(void);
const char *schwz_version(void);
/* threads the host-side setup loops run on (restricted_schwarz.cpp:56-304 is serial in the reference): SCHWZ_SETUP_THREADS,
 * else the smallest of the process's CPUs, its cgroup CPU quota and 32, divided among the ranks of a node when a
 * launcher says how many there are (LOCAL_WORLD_SIZE, OMPI_COMM_WORLD_LOCAL_SIZE, MPI_LOCALNRANKS).  Fixed at first use. */
int schwz_setup_threads(void);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int schwz_device_count(void);
/* device_guard (include/device_guard.hpp:47-101): bind the calling thread */
int schwz_set_device(int device);

/* ------------------------------------------------------------------------ */
/* 1. Stand-alone device kernels                                             */
/* ------------------------------------------------------------------------ */

/* Gather: into[i] = op(into[i], from[idx[i]])
 * replaces gather_kernel + gather_{,add_,diff_,avg_}values
 * (source/gather_kernel.cu:46-109, include/gather.hpp:70-142). */
int schwz_gather(int64_t n, const schwz_idx *d_idx, const double *d_from,
                 double *d_into, int op, schwz_stream stream);

/* Scatter: into[idx[i]] = op(into[idx[i]], from[i])
 * replaces scatter_kernel + launchers (source/scatter_kernel.cu:43-107,
 * include/scatter.hpp:70-143).  avg follows the CPU definition (y+x)/2. */
int schwz_scatter(int64_t n, const schwz_idx *d_idx, const double *d_from,
                  double *d_into, int op, schwz_stream stream);

/* The other instantiations of Gather / Scatter (source/gather_kernel.cu:112-146,
 * source/scatter_kernel.cu:109-142: {float, double, int, long} values x {int, long} indices); the hot
 * path itself only uses fp64 values with int32 indices (schwz_gather / schwz_scatter) and the fp32 wire
 * format of the mixed-precision halo. */
enum schwz_value_type { SCHWZ_VALUE_F32 = 0, SCHWZ_VALUE_F64 = 1, SCHWZ_VALUE_I32 = 2, SCHWZ_VALUE_I64 = 3 };
enum schwz_index_type { SCHWZ_INDEX_I32 = 0, SCHWZ_INDEX_I64 = 1 };
int schwz_gather_typed(int64_t n, const void *d_idx, int index_type, const void *d_from, void *d_into,
                       int value_type, int op, schwz_stream stream);
int schwz_scatter_typed(int64_t n, const void *d_idx, int index_type, const void *d_from, void *d_into,
                        int value_type, int op, schwz_stream stream);

/* CSR matrix resident in HBM, with the row-tile table the SpMV kernel needs.
 * Replaces gko::matrix::Csr<double,int> on the device executor.
 * The arrays are uploaded as they are.  SpMV sums every stored entry, but the preconditioned solvers read the
 * diagonal as ONE stored entry per row (Jacobi, block-Jacobi) and the symmetry check bisects the rows: a matrix
 * uploaded directly must hold every column once per row, ascending.  The problem sources of section 2
 * (schwz_problem_from_csr, schwz_problem_from_matrix_market) guarantee that for everything they feed. */
typedef struct schwz_csr schwz_csr;
int schwz_csr_create(int64_t nrows, int64_t ncols, const schwz_idx *h_row_ptr,
                     const schwz_idx *h_col, const double *h_val, schwz_csr **out);
void schwz_csr_destroy(schwz_csr *A);
int64_t schwz_csr_nnz(const schwz_csr *A);
/* encoding the default SpMV (variant 0) uses for this matrix: 0 = plain CSR, 1 = per-entry
 * dictionary tiles, 2 = row-pattern tiles, 3 = row-PAIR pattern tiles (lossless re-encodings
 * built at upload, csrc/spmv_dict.hip and csrc/spmv_pair.hip) */
int schwz_csr_format(const schwz_csr *A);
/* 1 when the upload found a row-pair coded matrix symmetric bit for bit and built the
 * upper-triangle tables the CG iteration takes p.(A p) from (about half the gathers of that
 * launch); such a matrix need not come from the reference's symmetric problems -- nothing is
 * assumed, the check runs on every upload.  0 otherwise. */
int schwz_csr_symmetric(const schwz_csr *A);
/* > 0 when the upload found the matrix to be a 3-D stencil in the canonical row-pair layout
 * {-PL, -NX, -1, 0, +1, +NX, +PL} and prepared the z-sweep walk of the CG update launch (bands of rows
 * swept through consecutive planes, operands from an LDS ring of plane windows; csrc/spmv_pair.hip):
 * the number of workgroup slots of that walk.  0: chunk-by-chunk gathers. */
int schwz_csr_sweep_slots(const schwz_csr *A);
/* chunks of 512 rows that walk leaves to a companion launch of the chunk-by-chunk kernel (rows whose
 * couplings do not fit the plane chains: 0 for a grid in natural order and for the slabs of its z-slab
 * partition, whose appended overlap planes are chained to the interior) */
int schwz_csr_sweep_left_out(const schwz_csr *A);
/* bytes of MATRIX data one SpMV pass reads in the coding `variant` launches (0: the coding the upload
 * chose, schwz_csr_format; anything else: plain CSR = 12 nnz + 4 (rows + 1), the figure of SURVEY 8(d)).
 * bench.py prices its roofline fraction on these bytes (+ the vector bytes of the launch). */
int64_t schwz_csr_matrix_bytes(const schwz_csr *A, int variant);

/* y = alpha*A*x + beta*y : gko Csr::apply(alpha,x,beta,y), call sites
 * source/restricted_schwarz.cpp:1014-1015, source/solve.cpp:834-835,1079-1080.
 * variant: 0 = default: the best coded tiles the matrix allows (row pairs, row patterns,
 * per-entry dictionaries; lossless, bit-identical results; see csrc/spmv_pair.hip,
 * csrc/spmv_dict.hip), else 6; 8 = row-pattern tiles, 7 = per-entry dictionary tiles,
 * 6 = plain CSR, LDS-staged row tiles with 16-byte batched loads,
 * 1 = one-row-per-lane baseline, 2 = first tiled version (scalar loads), 3/5 = wave-private
 * tiles (5: non-temporal matrix loads), 4 = software-pipelined tiles; 10.. = ablation builds
 * for tools/spmv_probe.py (deliberately wrong results). */
int schwz_csr_spmv(const schwz_csr *A, double alpha, const double *d_x,
                   double beta, double *d_y, int variant, schwz_stream stream);

/* Preconditioned CG on A x = b, device resident (no per-iteration host sync).
 * Replaces gko::solver::Cg + stop::Combined(Iteration, ResidualNormReduction)
 * as configured in source/solve.cpp:456-478,571-652 and applied by
 * SolverTools::solve_iterative_ginkgo (include/solver_tools.hpp:91-98).
 * x is the warm start on entry.  rtol<=0 runs exactly max_iters updates.
 * h_iters / h_resnorm (may be NULL) are written after an internal stream
 * sync only when requested. */
typedef struct schwz_pcg schwz_pcg;
int schwz_pcg_create(const schwz_csr *A, int precond, schwz_pcg **out);
/* the same with the block size of SCHWZ_PRECOND_BLOCK_JACOBI (metadata.precond_max_block_size,
 * 1..32) */
int schwz_pcg_create_ex(const schwz_csr *A, int precond, int block_size, schwz_pcg **out);
/* ILU / ISAI with the ParILU options of the reference's ParIlu (source/solve.cpp:506-532, :616-638):
 * par_ilu_sweeps > 0 computes the factors by that many ParILU sweeps on the GPU (schwz_parilu) instead of
 * the exact host ILU(0) (ilu and isai); trisolve_sweeps > 0 applies each factor by that many Jacobi passes
 * (schwz_trs_create_sweeps) instead of exact triangular solves (ilu only).  Both 0: schwz_pcg_create_ex.
 * Negative counts: SCHWZ_ERR_INVALID; a nonzero count with another preconditioner, or trisolve_sweeps
 * with isai: SCHWZ_ERR_NOT_IMPLEMENTED. */
int schwz_pcg_create_ilu(const schwz_csr *A, int precond, int par_ilu_sweeps, int trisolve_sweeps,
                         schwz_pcg **out);
void schwz_pcg_destroy(schwz_pcg *s);
/* how the last solve iterated (bench.py needs it to name and price its launches): bits 0-1: 0 = q = A p
 * stored, 1 = q-free, three launches per iteration, 2 = q-free with the direction update fused into the
 * next iteration's p.(A p) launch (two launches); 4: x += sum alpha_k p_k deferred; 8 / 16: the update /
 * the fused launch walked the matrix in z-sweeps (csrc/spmv_pair.hip); 32: so did the start residual and
 * the first direction of the solve */
int schwz_pcg_flavour(const schwz_pcg *s);
int schwz_pcg_solve(schwz_pcg *s, const double *d_b, double *d_x, double rtol,
                    int max_iters, int *h_iters, double *h_resnorm,
                    schwz_stream stream);

/* Mixed-precision CG (an extension: the reference's only mixed-precision feature is the fp32 halo): the solve runs
 * in residual-correction form,
 *   1. r0 = b - A x in fp64, through the matrix's best fp64 coding, nu = ||r0||_2;
 *   2. nu == 0: x is untouched, 0 iterations;
 *   3. PCG on A32 e = fl32(r0 / nu) from e = 0, with fp32 matrix values (a copy of 4 nnz bytes built at creation,
 *      round to nearest) and fp32 vectors; dot products and norms are accumulated in fp64, in a fixed order (the
 *      same input gives the same bits); the stop rule is schwz_pcg_solve's, on the recurred residual relative to
 *      the norm of the scaled start residual;
 *   4. x += nu e in fp64.
 * One step of iterative refinement: a caller that recomputes the residual in fp64 and calls again (the RAS
 * iteration does) reaches fp64 accuracy.  h_resnorm is nu times the recurred norm.  precond: SCHWZ_PRECOND_NONE
 * or SCHWZ_PRECOND_JACOBI; another known code: SCHWZ_ERR_NOT_IMPLEMENTED; an unknown code or a null `out`:
 * SCHWZ_ERR_INVALID (both checked before the matrix is looked at).  A finite matrix value that rounds to
 * +-inf in fp32: SCHWZ_ERR_NOT_IMPLEMENTED, the message names the entry.  Plain CSR only (csrc/cg_f32.hip): the
 * codings and the z-sweep walk have no fp32 form, so on a stencil matrix this solver moves MORE bytes than
 * schwz_pcg does. */
typedef struct schwz_pcg_f32 schwz_pcg_f32;
int schwz_pcg_f32_create(const schwz_csr *A, int precond, schwz_pcg_f32 **out);
void schwz_pcg_f32_destroy(schwz_pcg_f32 *s);
int schwz_pcg_f32_solve(schwz_pcg_f32 *s, const double *d_b, double *d_x, double rtol, int max_iters,
                        int *h_iters, double *h_resnorm, schwz_stream stream);
/* q = A32 p and, through *h_pq (may be NULL), p.q as the iteration accumulates it, by the launch the iteration
 * uses: for tests and probes.  d_p, d_q: n floats in HBM.  Synchronises `stream`; not to be called between the
 * launch of a solve on another stream and its end. */
int schwz_pcg_f32_spmv(schwz_pcg_f32 *s, const float *d_p, float *d_q, double *h_pq, schwz_stream stream);
/* iterations and residual norm of the last solve (device synchronisation) */
int schwz_pcg_f32_last_stats(schwz_pcg_f32 *s, int *h_iters, double *h_resnorm);

/* Restarted GMRES(restart) with right preconditioning, device resident like the CG.
 * Replaces gko::solver::Gmres with krylov_dim = settings.restart_iter and the same
 * Combined(Iteration, ResidualNormReduction) criterion, the local solver of
 * settings.non_symmetric_matrix (source/solve.cpp:486-520, applied at :750-753).
 * max_iters counts Krylov vectors over all cycles; h_resnorm is the residual norm the
 * stop test saw (the rotated right-hand side inside a cycle). */
typedef struct schwz_gmres schwz_gmres;
int schwz_gmres_create(const schwz_csr *A, int precond, int block_size, int restart, schwz_gmres **out);
/* the same with the ParILU options of schwz_pcg_create_ilu (both 0: schwz_gmres_create) */
int schwz_gmres_create_ex(const schwz_csr *A, int precond, int block_size, int restart, int par_ilu_sweeps,
                          int trisolve_sweeps, schwz_gmres **out);
/* The same with the type the Krylov basis is stored in (an extension: compressed-basis GMRES).
 * SCHWZ_GMRES_BASIS_F64 is schwz_gmres_create_ex, launch for launch.  SCHWZ_GMRES_BASIS_F32 stores every basis
 * vector rounded to fp32 (4 (restart + 1) n bytes instead of 8) and orthogonalises by blocked classical
 * Gram-Schmidt applied twice, in three passes over the basis and a constant number of launches per Krylov vector;
 * all arithmetic, the matrix, the preconditioner, the Hessenberg matrix and x stay fp64, and the rounded vector is
 * the one the next matrix-vector product sees, so the Arnoldi relation holds for the stored basis.  Caveat: the
 * stop test inside a cycle is on the RECURRED norm (the rotated right-hand side).  The start residual of a cycle
 * is itself only represented to fp32 accuracy (r = beta fl32(r / beta) + O(2^-24 beta)), so within ONE cycle the
 * true residual follows the recurred one only down to about 2^-24 of that cycle's start residual; every restart
 * recomputes the residual in fp64.  Restarted runs need the iterations of the fp64 basis; a reduction far beyond
 * 2^-24 inside a single long cycle takes more iterations (or another cycle), never a wrong answer.  restart up to
 * 2048 as for fp64.  SCHWZ_ERR_INVALID for an unknown basis code. */
enum schwz_gmres_basis { SCHWZ_GMRES_BASIS_F64 = 0, SCHWZ_GMRES_BASIS_F32 = 1 };
int schwz_gmres_create_basis(const schwz_csr *A, int precond, int block_size, int restart, int par_ilu_sweeps,
                             int trisolve_sweeps, int basis, schwz_gmres **out);
/* the basis type of a solver (SCHWZ_GMRES_BASIS_F64 for NULL) */
int schwz_gmres_basis(const schwz_gmres *s);
void schwz_gmres_destroy(schwz_gmres *s);
int schwz_gmres_solve(schwz_gmres *s, const double *d_b, double *d_x, double rtol, int max_iters,
                      int *h_iters, double *h_resnorm, schwz_stream stream);
/* iterations and residual norm of the last solve (device synchronisation) */
int schwz_gmres_last_stats(schwz_gmres *s, int *h_iters, double *h_resnorm);

/* BiCGSTAB with right preconditioning (van der Vorst 1992), device resident like the CG and GMRES: a second
 * local solver for non-symmetric matrices, an extension (the reference offers GMRES only).  Two matrix-vector
 * products and five vector launches per iteration, 8 work vectors whatever the iteration count.  The
 * preconditioner codes and the ParILU options are those of schwz_gmres_create_ex.  The solve stops before
 * iteration k when k == max_iters or the recurred residual norm ||r_k|| is <= rtol times the start residual norm
 * (or exactly zero), and in the middle of an iteration when ||s|| is (the half step is then applied and counts as
 * an iteration); rtol <= 0 runs exactly max_iters iterations unless a norm is exactly zero or the recurrence
 * breaks down.  h_resnorm is the recurred norm the stop test saw, not the norm of b - A x.  A breakdown ends the
 * solve with a finite x and SCHWZ_OK; schwz_bicgstab_breakdown tells which (device synchronisation): 0 none,
 * 1 rho = 0 at the top, 2 rhat.v = 0 (x untouched by that iteration), 3 t.t = 0 or t.s = 0 (half step applied);
 * -1 when the device state could not be read (schwz_last_error says why), 0 for a null solver.
 * The host looks at the device state every SCHWZ_BICGSTAB_POLL_BATCH iterations, one batch behind the launches. */
#define SCHWZ_BICGSTAB_POLL_BATCH 8
typedef struct schwz_bicgstab schwz_bicgstab;
int schwz_bicgstab_create(const schwz_csr *A, int precond, int block_size, int par_ilu_sweeps, int trisolve_sweeps,
                          schwz_bicgstab **out);
void schwz_bicgstab_destroy(schwz_bicgstab *s);
int schwz_bicgstab_solve(schwz_bicgstab *s, const double *d_b, double *d_x, double rtol, int max_iters,
                         int *h_iters, double *h_resnorm, schwz_stream stream);
/* iterations and residual norm of the last solve (device synchronisation) */
int schwz_bicgstab_last_stats(schwz_bicgstab *s, int *h_iters, double *h_resnorm);
int schwz_bicgstab_breakdown(schwz_bicgstab *s);

/* Chebyshev iteration for SPD matrices (an extension: the reference's symmetric local solver is CG only), device
 * resident, one reduction-free launch per iteration (csrc/chebyshev.hip).  With M = I (SCHWZ_PRECOND_NONE) or
 * M = diag(A) (SCHWZ_PRECOND_JACOBI), the spectrum of M^-1 A assumed in [lmin, lmax]:
 *   theta = (lmax + lmin) / 2 ; delta = (lmax - lmin) / 2 ; sigma = theta / delta
 *
 *   r_0 = b - A x_0 ;  rho_0 = 1 / sigma ;  d_0 = (1 / theta) M^-1 r_0
 *   for k = 0 ... m-1:
 *       x_{k+1} = x_k + d_k
 *       r_{k+1} = r_k - A d_k
 *       rho_{k+1} = 1 / (2 sigma - rho_k)
 *       d_{k+1} = (rho_{k+1} rho_k) d_k + (2 rho_{k+1} / delta) M^-1 r_{k+1}
 *
 * max_iters = m is the number of corrections applied, the polynomial degree.  The scalars are computed on the host in
 * fp64, in exactly the order written above, and passed to the launches by value.  The iteration converges for any
 * 0 < lmin < lmax as long as lmax really is an upper bound (eigenvalues below lmin are still damped, only more
 * slowly); a lmax below the true one makes it DIVERGE.  At creation lmax is the Gershgorin bound
 * max_i |1 / m_ii| sum_j |a_ij|, which is guaranteed, and lmin = lmax / 30, the conventional default eigenvalue ratio
 * of Chebyshev smoothers (hypre, Ifpack2, PETSc): a default, not a measurement.  Better bounds are the caller's
 * responsibility (schwz_cheb_set_bounds: 0 < lmin < lmax, both finite, else SCHWZ_ERR_INVALID; they take effect from
 * the next solve).
 * create: precond SCHWZ_PRECOND_NONE or SCHWZ_PRECOND_JACOBI; another known code: SCHWZ_ERR_NOT_IMPLEMENTED; an
 * unknown code or a null `out`: SCHWZ_ERR_INVALID (both checked before the matrix is looked at).  With Jacobi a row
 * whose diagonal is missing, zero, negative or not finite: SCHWZ_ERR_NOT_SPD.  The solver reads plain CSR, whatever
 * coding the upload chose.
 * solve, rtol <= 0 (fixed work): the start launch, m - 1 iteration launches and one vector launch, m matrix passes;
 * the host polls nothing and no launch reads device state; m = 0 launches nothing and leaves x untouched.  The norm
 * ||r_m|| costs one more matrix pass and is computed only when asked for (a non-NULL h_resnorm: on `stream`;
 * schwz_cheb_last_stats: behind its device synchronisation), once; that pass stores nothing to x or the work
 * vectors.  After max_iters = 0 without h_resnorm, last_stats reports a NaN norm (b and x are the caller's).
 * solve, rtol > 0: ||r_k|| is looked at for k = 0 (mod SCHWZ_CHEB_CHECK_EVERY) and for k = m, and the solve returns
 * x_k for the first such k with ||r_k|| <= rtol ||r_0|| or ||r_k|| = 0 (k = m if none): iterations are reported in
 * {0, 8, 16, ..., m}.  A zero start residual means 0 iterations and x untouched.  h_resnorm is the recurred norm. */
#define SCHWZ_CHEB_CHECK_EVERY 8
typedef struct schwz_cheb schwz_cheb;
int schwz_cheb_create(const schwz_csr *A, int precond, schwz_cheb **out);
void schwz_cheb_destroy(schwz_cheb *s);
int schwz_cheb_bounds(const schwz_cheb *s, double *lmin, double *lmax);
int schwz_cheb_set_bounds(schwz_cheb *s, double lmin, double lmax);
int schwz_cheb_solve(schwz_cheb *s, const double *d_b, double *d_x, double rtol, int max_iters,
                     int *h_iters, double *h_resnorm, schwz_stream stream);
/* iterations and residual norm of the last solve (device synchronisation) */
int schwz_cheb_last_stats(schwz_cheb *s, int *h_iters, double *h_resnorm);

/* ---- Block vectors: K right-hand sides against one matrix (an extension: the reference solves one system, so no
 * line of it is replaced; csrc/batch.hip).  A block vector of n rows and k columns is stored row-interleaved, element
 * (i, j) at i * k + j, k = 2, 4 or 8 -- any other k: SCHWZ_ERR_INVALID, checked before anything else.  The kernels
 * read plain CSR, whatever coding the upload chose for the single-vector path: values and columns come from HBM once
 * per tile, independent of k, and every row sum runs in CSR order without contraction, so column j of a result
 * depends on column j of the operands alone, bit for bit.  All entry points obey `stream`.
 *
 * schwz_csr_spmm: Y = alpha A X + beta Y (beta == 0: Y is not read).  X holds ncols * k values, Y nrows * k.
 *
 * schwz_bcg: k independent CG recurrences that share the matrix pass, fp64, precond SCHWZ_PRECOND_NONE or
 * SCHWZ_PRECOND_JACOBI (another known code: SCHWZ_ERR_NOT_IMPLEMENTED; an unknown one, a null `out`, a matrix that is
 * not square: SCHWZ_ERR_INVALID; with Jacobi a row without a positive finite diagonal entry: SCHWZ_ERR_NOT_SPD).
 * alpha_j, beta_j and the freeze mask stay on the device; an iteration is three launches (Q = A P with the partial
 * sums of p.q; the update of x and r; the direction), and every reduction is a set of per-workgroup partial sums the
 * next launch folds in a fixed order.
 * solve: X is the warm start on entry.  Column j is FROZEN -- its x_j and r_j stop changing, bit for bit -- once
 * ||r_j|| <= rtol ||r_0,j|| (the loop-top test of schwz_pcg_solve, per column), where r_0,j = 0, p_j.q_j = 0 or
 * r_j.z_j = 0 would be divided by (a zero column stays exactly zero), and from the first launch on where bit j of
 * `frozen` is set (bits >= k: SCHWZ_ERR_INVALID).  rtol <= 0: exactly max_iters iterations are launched, the host
 * polls nothing.  rtol > 0: the solve ends when every column is frozen or at max_iters; the host polls the pinned copy
 * of the state one chunk of launches behind, as schwz_cheb_solve does, and launches past the stop return at once.
 * h_iters / h_resnorm (k values each; may be NULL) are the updates applied to each column and the recurred residual
 * norms, written behind a synchronisation of `stream` only when asked for; schwz_bcg_last_stats reports the same at
 * any later time (device synchronisation).
 * schwz_bcg_residual: h_norm_sq[j] = ||b_j - A x_j||^2 (k values; waits for `stream`), and R = B - A X stored to d_r
 * where d_r is not NULL (NULL: the norm-only form, nothing stored).  Uses the solver's scratch: not beside a solve of
 * the same object on another stream. */
typedef struct schwz_bcg schwz_bcg;
int schwz_csr_spmm(const schwz_csr *A, int k, double alpha, const double *d_x, double beta, double *d_y,
                   schwz_stream stream);
int schwz_bcg_create(const schwz_csr *A, int precond, int k, schwz_bcg **out);
void schwz_bcg_destroy(schwz_bcg *s);
int schwz_bcg_solve(schwz_bcg *s, const double *d_b, double *d_x, double rtol, int max_iters, unsigned frozen,
                    int *h_iters, double *h_resnorm, schwz_stream stream);
int schwz_bcg_last_stats(schwz_bcg *s, int *h_iters, double *h_resnorm);
int schwz_bcg_residual(schwz_bcg *s, const double *d_b, const double *d_x, double *d_r, double *h_norm_sq,
                       schwz_stream stream);

/* Profiling hooks for bench.py's roofline leg: between begin and end, every
 * launch of the dominant kernel (the CSR SpMV inside schwz_pcg_solve) is
 * bracketed by a HIP event pair on its launch stream; end synchronises and
 * returns the summed kernel time and the launch count.  Replaces nothing in
 * the reference (its MEASURE_ELAPSED_FUNC_TIME, include/settings.hpp:508-523,
 * times host calls without a device sync). */
int schwz_profile_begin(int capacity);
/* STREAM-style probe for the measured HBM ceiling quoted beside the 8 TB/s spec
 * (SURVEY 8d): mode 0 copies n doubles src->dst in a grid-stride loop of 2048
 * persistent workgroups, mode 1 reads n doubles and writes one partial sum per
 * workgroup (dst needs 2048 doubles), mode 2 copies with one 16-byte element
 * per thread and a grid that covers the buffer once (the form that reaches the
 * ~6.2 TB/s copy ceiling), mode 3 / 4 four elements per thread, plain /
 * non-temporal. */
int schwz_stream_probe(int64_t n, int mode, const double *d_src, double *d_dst,
                       schwz_stream stream);
int schwz_profile_end(double *h_total_ms, int64_t *h_launches);
/* after schwz_profile_end: the same figures per launch kind of a CG iteration, 0 = the SpMV (+ p.Ap)
 * launch, 1 = the fused recompute-and-update launch of the q-free iteration (zero launches when the
 * solver stores q) */
int schwz_profile_kind(int kind, double *h_total_ms, int64_t *h_launches);

/* Sparse triangular solves y = P^T L^-T L^-1 P b.
 * Replaces gko::solver::LowerTrs/UpperTrs + Permutation::apply as used by
 * Solve::local_solve (source/solve.cpp:709-720) and
 * SolverTools::solve_direct_ginkgo (include/solver_tools.hpp:69-87); also the
 * intent of the dead CusparseWrappers (include/cusparse_helpers.hpp:200-212).
 * L: CSR lower, diagonal last in each row; U: CSR upper, diagonal first (U = L^T for the
 * Cholesky path; any L, U pair for ILU).  h_perm may be NULL (identity).  Factors whose level
 * structure does not fit one workgroup are solved level by level with multi-workgroup launches. */
typedef struct schwz_trs schwz_trs;
int schwz_trs_create(int64_t n, const schwz_idx *h_l_rp, const schwz_idx *h_l_col,
                     const double *h_l_val, const schwz_idx *h_u_rp,
                     const schwz_idx *h_u_col, const double *h_u_val,
                     const schwz_idx *h_perm, schwz_trs **out);
/* The LU variant: y[h_col_perm[i]] = (U^-1 L^-1 w)[i] with w[i] = b[h_row_perm[i]], i.e.
 * y = Q U^-1 L^-1 P b for A(row_perm, col_perm) = L U (schwz_lu).  Same factor layout as above;
 * both permutations are required.  Factors beyond the one-workgroup kernel whose rows exceed 64
 * entries (LU fill of a banded subdomain) are swept by a flag-driven kernel with one wave per row. */
int schwz_trs_create_lu(int64_t n, const schwz_idx *h_l_rp, const schwz_idx *h_l_col,
                        const double *h_l_val, const schwz_idx *h_u_rp,
                        const schwz_idx *h_u_col, const double *h_u_val,
                        const schwz_idx *h_row_perm, const schwz_idx *h_col_perm,
                        schwz_trs **out);
/* The Jacobi-sweep mode (the triangular solves Ginkgo's ParIlu preconditioner can run instead of exact sweeps,
 * source/solve.cpp:506-532): each factor T = D + T_s is applied by `sweeps` (>= 1) Jacobi passes,
 * x_0 = D^-1 b, x_{m+1} = D^-1 (b - T_s x_m), i.e. y = sum_{m=0..k} (-D^-1 T_s)^m D^-1 b -- exact once
 * sweeps >= levels - 1 of the factor.  No permutation; same factor layout as schwz_trs_create (any nonzero
 * diagonals).  One launch per pass, no level plan, no waits between workgroups (csrc/parilu.hip). */
int schwz_trs_create_sweeps(int64_t n, const schwz_idx *h_l_rp, const schwz_idx *h_l_col,
                            const double *h_l_val, const schwz_idx *h_u_rp,
                            const schwz_idx *h_u_col, const double *h_u_val, int sweeps,
                            schwz_trs **out);
/* passes per factor of a triangular-solve object in the sweep mode; 0: exact solves */
int schwz_trs_sweeps(const schwz_trs *t);
void schwz_trs_destroy(schwz_trs *t);
int schwz_trs_solve(schwz_trs *t, const double *d_b, double *d_y, schwz_stream stream);

/* ParILU on the GPU: gko::factorization::ParIlu (source/solve.cpp:506-532, and the factors of
 * Ilu<LowerIsai, UpperIsai>, :616-638) as `sweeps` (>= 1) SYNCHRONOUS fixed-point sweeps on the ILU(0)
 * pattern of A (Ginkgo sweeps asynchronously in place; the synchronous form is reproducible).  Start:
 * L0 = strict lower part of A with a unit diagonal, U0 = upper part of A; one sweep sets
 *   l_ij = (a_ij - sum_{k<j} l_ik u_kj) / u_jj  (i > j),   u_ij = a_ij - sum_{k<i} l_ik u_kj  (i <= j)
 * from the previous iterate.  Once sweeps reaches the longest dependency chain among the entries the
 * factors are those of schwz_ilu0 (up to rounding).  Same layout as schwz_ilu0: L unit lower with the 1
 * LAST in each row, U upper with its diagonal FIRST.  A's columns must be sorted with the diagonal
 * present.  A zero or non-finite u_ii after the last sweep returns SCHWZ_ERR_NOT_SPD.
 * schwz_parilu reads A in HBM (only its pattern comes back, for the symbolic pass); the patterns are
 * malloc'd host arrays (schwz_free), the values device arrays (schwz_device_free).  Synchronous.
 * schwz_parilu_host: schwz_ilu0's signature plus `sweeps`, runs on the GPU, all outputs malloc'd. */
int schwz_parilu(const schwz_csr *A, int sweeps, schwz_idx **l_rp, schwz_idx **l_col, double **d_l_val,
                 schwz_idx **u_rp, schwz_idx **u_col, double **d_u_val);
int schwz_parilu_host(int64_t n, const schwz_idx *h_rp, const schwz_idx *h_col, const double *h_val,
                      int sweeps, schwz_idx **l_rp, schwz_idx **l_col, double **l_val, schwz_idx **u_rp,
                      schwz_idx **u_col, double **u_val);
void schwz_device_free(void *d_ptr);

/* ------------------------------------------------------------------------ */
/* 2. Host-side setup (no GPU needed)                                        */
/* ------------------------------------------------------------------------ */

/* Global problem description: either an explicit CSR or an analytic stencil
 * whose rows are produced on demand, so that no rank ever holds a global
 * matrix (the reference replicates it, source/schwarz_base.cpp:142-147). */
typedef struct schwz_problem schwz_problem;

/* Initialize::setup_global_matrix, Laplacian branch
 * (source/initialization.cpp:214-265): dim=2 is the reference's 5-point
 * stencil on an nx*nx grid; dim=3 is the 7-point extension on nx*ny*nz. */
int schwz_problem_laplacian(int dim, int64_t nx, int64_t ny, int64_t nz,
                            schwz_problem **out);
/* explicit CSR with int64 row_ptr (copied).  The arrays are checked before anything is read through them:
 * h_row_ptr[0] != 0, a row_ptr that decreases or is negative anywhere, a column < 0 or >= N: SCHWZ_ERR_INVALID.
 * Rows may be unsorted (deal.II stores the diagonal first): they are stable-sorted by column.  Rows may hold a
 * column more than once: those entries are summed in their stored order and stored once.  The pattern does not
 * depend on the values (explicit zeros, and sums that vanish, stay stored).  Every problem therefore has
 * strictly ascending columns in every row. */
int schwz_problem_from_csr(int64_t N, const int64_t *h_row_ptr,
                           const schwz_idx *h_col, const double *h_val,
                           schwz_problem **out);
/* Distributed ingest: the reference reads the whole file on every rank and keeps the whole matrix there
 * (initialization.cpp:204-213).  Here one rank may parse and partition, cut out what every
 * subdomain reads -- its interior and overlap rows, schwz_problem_extract_rows -- and hand each rank a row
 * source that holds only that part (row ids ascending, CSR over those rows, columns global and ascending);
 * schwz_subdomain_setup on it gives the same subdomain as on the whole matrix and fails if it needs a row
 * that is not there.  extract_rows: first call with h_col == NULL fills h_row_ptr (nrows + 1 entries).
 * from_rows sorts and sums nothing: row ids that are not strictly ascending or lie outside [0, N), a row_ptr that
 * does not start at 0 or decreases anywhere, columns that are not strictly ascending or lie outside [0, N):
 * SCHWZ_ERR_INVALID (what extract_rows hands out always passes). */
int schwz_problem_from_rows(int64_t N, int64_t nrows, const int64_t *h_row_ids, const int64_t *h_row_ptr,
                            const schwz_idx *h_col, const double *h_val, schwz_problem **out);
int schwz_problem_extract_rows(const schwz_problem *p, int64_t nrows, const int64_t *h_row_ids,
                               int64_t *h_row_ptr, schwz_idx *h_col, double *h_val);
/* Matrix-Market file branch (initialization.cpp:204-213): gko::read +
 * sort_by_column_index.  The banner is the five words "%%MatrixMarket matrix coordinate <field> <symmetry>" in
 * any letter case, field real | integer | pattern, symmetry general | symmetric | skew-symmetric; array, complex,
 * hermitian, any other word and a missing banner are refused.  Comment lines ('%') before the size line and blank
 * lines anywhere are skipped; LF or CRLF.  The matrix must be square with 1 <= n < 2^31 - 1.  Every entry line
 * holds exactly "row col value" ("row col" in a pattern file, value 1.0), indices 1-based inside the matrix, the
 * value wholly a finite number (an integer in an integer file).  symmetric and skew-symmetric files hold the lower
 * triangle only (skew-symmetric: no diagonal entry); the mirror of (i, j, v) is (j, i, v), skew-symmetric
 * (j, i, -v).  Entries of one (row, col) are summed in file order and stored once (schwz_problem_from_csr).
 * Refused with SCHWZ_ERR_IO and a message that names the entry or the word: an index outside the matrix, an
 * entry line with another number of fields, a value that is not a finite number, an entry above the diagonal or on
 * the diagonal of a skew-symmetric file, fewer entries than the size line announces, content after the last one,
 * a negative count.  Nothing is allocated from the announced count beyond what the bytes of the file can hold. */
int schwz_problem_from_matrix_market(const char *path, schwz_problem **out);
void schwz_problem_destroy(schwz_problem *p);
int64_t schwz_problem_size(const schwz_problem *p);
int64_t schwz_problem_nnz(const schwz_problem *p);
/* copy one row out (count returned through *n; cols ascending) */
int schwz_problem_row(const schwz_problem *p, int64_t row, int *n,
                      int64_t *cols, double *vals, int capacity);
/* Apply a partition vector: A <- A(perm,perm) with perm grouping rows by
 * part id, stable within a part (source/restricted_schwarz.cpp:105-152).
 * h_perm (new->old, length N) and first_row (P+1) are outputs. */
int schwz_problem_permute(const schwz_problem *p, int P, const uint32_t *h_part,
                          int64_t *h_perm, int64_t *h_first_row,
                          schwz_problem **out);

/* Initialize::generate_rhs (source/initialization.cpp:88-96): entry g of the sequence
 * std::uniform_real_distribution<double>(0,1) draws from a default-seeded
 * std::default_random_engine (libstdc++: minstd_rand0, two draws per value).  Random access by
 * global row id (LCG jump-ahead), so no rank generates or broadcasts the whole vector
 * (source/schwarz_base.cpp:169-182 does). */
int schwz_rhs_random(int64_t count, const int64_t *h_global_ids, double *h_out);
/* contiguous row blocks (source/restricted_schwarz.cpp:84,97-102) */
int schwz_partition_regular(int64_t N, int P, int64_t *h_first_row);
/* PartitionTools::PartitionRegular2D (include/partition_tools.hpp:70-106) */
int schwz_partition_regular2d(int64_t n1d, int P, uint32_t *h_part);
/* graph partition standing in for PartitionTools::PartitionMetis
 * (include/partition_tools.hpp:110-202; METIS itself is absent): multilevel
 * recursive bisection of the (symmetrised) matrix graph -- heavy-edge
 * coarsening, greedy growing on the coarsest graph, Fiduccia-Mattheyses
 * refinement on every level -- to part sizes that differ by at most one row.
 * Deterministic.  SCHWZ_PART_MULTILEVEL=0: the single-level bisection of
 * rounds 1-2. */
int schwz_partition_graph(const schwz_problem *p, int P, uint32_t *h_part);

/* Subdomain: index sets, local/interface matrices, comm lists, device state.
 * SolverRAS::setup_local_matrices (source/restricted_schwarz.cpp:56-304) and
 * setup_comm_buffers (:308-604). */
typedef struct schwz_subdomain schwz_subdomain;

/* h_first_row: P + 1 entries from 0 to N that never decrease, else SCHWZ_ERR_INVALID. */
int schwz_subdomain_setup(const schwz_problem *p, int P, int me, int overlap,
                          const int64_t *h_first_row, schwz_subdomain **out);
void schwz_subdomain_destroy(schwz_subdomain *sd);

/* sizes[0]=local_size [1]=local_size_x [2]=overlap_size [3]=halo_size
 * [4]=nnz_local [5]=nnz_interface [6]=num_neighbors_in [7]=num_neighbors_out
 * [8]=num_recv [9]=num_send  (Metadata fields, include/settings.hpp:318-496) */
int schwz_subdomain_sizes(const schwz_subdomain *sd, int64_t *sizes10);
/* local id -> global id, length local_size_x + halo_size */
int schwz_subdomain_local_to_global(const schwz_subdomain *sd, int64_t *h_out);
/* local_matrix / interface_matrix on the host (interface columns are
 * returned as GLOBAL ids, like the reference stores them) */
int schwz_subdomain_local_matrix(const schwz_subdomain *sd, schwz_idx *h_rp,
                                 schwz_idx *h_col, double *h_val);
int schwz_subdomain_interface_matrix(const schwz_subdomain *sd, schwz_idx *h_rp,
                                     int64_t *h_col_global, double *h_val);
/* comm_struct.neighbors_in / global_get (include/communicate.hpp:67-224):
 * k-th in-neighbour; ids ascending global */
int schwz_subdomain_get_list(const schwz_subdomain *sd, int k, int *rank,
                             int64_t *count, int64_t *h_ids /* may be NULL */);
/* the index handshake of restricted_schwarz.cpp:400-472: neighbour p's get
 * list for me is my put list for p.  Add in ascending p. */
int schwz_subdomain_add_put_list(schwz_subdomain *sd, int p, int64_t count,
                                 const int64_t *h_ids);
int schwz_subdomain_put_list(const schwz_subdomain *sd, int k, int *rank,
                             int64_t *count, int64_t *h_ids /* may be NULL */);
/* offsets of neighbour k inside the packed send / recv buffers (prefix sums in
 * neighbour order, restricted_schwarz.cpp:870,909,913,940) */
int schwz_subdomain_send_offset(const schwz_subdomain *sd, int k, int64_t *offset);
int schwz_subdomain_recv_offset(const schwz_subdomain *sd, int k, int64_t *offset);

/* Host sparse LL^T of the local matrix, standing in for CHOLMOD simplicial
 * LL^T (Solve::compute_local_factors, source/solve.cpp:75-143): identity
 * A(perm,perm) = L L^T.  Outputs are malloc'd; free with schwz_free.
 * schwz_cholesky, schwz_lu and schwz_isai, like schwz_ilu0: rows whose columns are not strictly ascending
 * (unsorted, or a column stored twice) or lie outside [0, n): SCHWZ_ERR_INVALID.  No exception leaves a function
 * of this section: an allocation that fails, or a length no container holds, is SCHWZ_ERR_INVALID too. */
int schwz_cholesky(int64_t n, const schwz_idx *h_rp, const schwz_idx *h_col,
                   const double *h_val, int natural_ordering, schwz_idx **l_rp,
                   schwz_idx **l_col, double **l_val, schwz_idx **u_rp,
                   schwz_idx **u_col, double **u_val, schwz_idx **perm);
/* Host sparse LU with threshold partial pivoting, standing in for UMFPACK (Solve::compute_local_factors
 * with factorization == "umfpack", source/solve.cpp:144-173,321-390): A(row_perm, col_perm) = L U,
 * L unit lower with the 1 stored LAST in each row, U upper with its diagonal FIRST, columns sorted
 * -- the layout schwz_trs_create_lu expects.  Columns are pre-ordered by reverse Cuthill-McKee on
 * the pattern of A + A^T (identity when natural_ordering is set); left-looking Gilbert-Peierls;
 * the pivot of a column is the pre-order's diagonal entry when |a| >= 0.1 * max|column|
 * (UMFPACK's default tolerance), else the largest entry.  NO row scaling: the reference hands
 * UMFPACK's L and U to the triangular solves without the row-scale vector, which is exact only
 * when scaling is off; here the factors are those of A itself.  A column without a nonzero pivot
 * candidate returns SCHWZ_ERR_NOT_SPD.  Outputs are malloc'd; free with schwz_free. */
int schwz_lu(int64_t n, const schwz_idx *h_rp, const schwz_idx *h_col, const double *h_val,
             int natural_ordering, schwz_idx **l_rp, schwz_idx **l_col, double **l_val,
             schwz_idx **u_rp, schwz_idx **u_col, double **u_val, schwz_idx **row_perm,
             schwz_idx **col_perm);
/* Host ILU(0) on the pattern of A (columns sorted): L unit lower with the 1 stored LAST in each
 * row, U upper with its diagonal FIRST -- the layout schwz_trs_create expects.  Stands in for
 * gko::factorization::ParIlu (source/solve.cpp:506-532), whose sweeps converge to these
 * factors.  Outputs are malloc'd; free with schwz_free. */
int schwz_ilu0(int64_t n, const schwz_idx *h_rp, const schwz_idx *h_col, const double *h_val,
               schwz_idx **l_rp, schwz_idx **l_col, double **l_val, schwz_idx **u_rp,
               schwz_idx **u_col, double **u_val);
/* Incomplete sparse approximate inverse of a triangular CSR factor on the factor's own pattern:
 * row i of W solves W(i,S) T(S,S) = e_i(S), S = pattern of row i of T.  Replaces
 * gko::preconditioner::LowerIsai / UpperIsai with sparsity power 1 (source/solve.cpp:616-638).
 * *w_val (nnz(T) values on T's pattern) is malloc'd; free with schwz_free. */
int schwz_isai(int64_t n, const schwz_idx *h_rp, const schwz_idx *h_col, const double *h_val, int lower,
               double **w_val);
void schwz_free(void *p);

/* ------------------------------------------------------------------------ */
/* 3. Device-resident RAS iteration of one subdomain                         */
/* ------------------------------------------------------------------------ */

typedef struct {
    int32_t local_solver;    /* schwz_local_solver */
    int32_t precond;         /* schwz_precond */
    double local_tol;        /* metadata.local_solver_tolerance */
    int32_t local_max_iters; /* -1 => local_size_x (solve.cpp:458-463) */
    int32_t natural_factor_ordering; /* settings.naturally_ordered_factor */
    int32_t spmv_variant;    /* 0 default (the best coding the matrix allows); see schwz_csr_spmv */
    int32_t precond_block_size; /* metadata.precond_max_block_size (block-jacobi) */
    int32_t non_symmetric;   /* settings.non_symmetric_matrix: GMRES instead of CG */
    int32_t restart_iter;    /* settings.restart_iter (GMRES krylov_dim), >= 1 */
    /* ParILU options of the iterative local solver (schwz_pcg_create_ilu); 0 = exact ILU(0) / exact
     * triangular solves.  Nonzero only with SCHWZ_SOLVER_ITERATIVE and precond ilu (both) or isai
     * (par_ilu_sweeps), else SCHWZ_ERR_NOT_IMPLEMENTED; negative: SCHWZ_ERR_INVALID. */
    int32_t par_ilu_sweeps;
    int32_t trisolve_sweeps;
} schwz_solver_options;

/* Upload matrices / index lists, allocate x~=[interior|overlap|halo] (zero,
 * SURVEY F9), local rhs, CG work vectors; factor on the host for the direct
 * path.  h_local_rhs has local_size_x entries: [rhs[interior]; rhs[overlap_row]]
 * (Initialize::setup_vectors, source/initialization.cpp:332-359).
 * Requires all put lists to be set.  Binds to the current HIP device. */
int schwz_subdomain_to_device(schwz_subdomain *sd, const double *h_local_rhs,
                              const schwz_solver_options *opt);

/* step 0a: send[off_k + i] = x~[put_k[i]] for every out-neighbour
 * (exchange_boundary_twosided pack half, restricted_schwarz.cpp:884-911;
 * CommHelpers::pack_buffer, include/comm_helpers.hpp:93-118).
 * d_send has num_send entries. */
int schwz_ras_pack(schwz_subdomain *sd, double *d_send, schwz_stream stream);
/* step 0b: x~[get_k[i]] = recv[off_k + i] for every in-neighbour
 * (restricted_schwarz.cpp:950-962; CommHelpers::unpack_buffer,
 * include/comm_helpers.hpp:154-177).  d_recv has num_recv entries. */
int schwz_ras_unpack(schwz_subdomain *sd, const double *d_recv, schwz_stream stream);
/* Mixed-precision variants of step 0 (settings.use_mixed_precision with MixedValueType =
 * float): the packed halo travels as fp32 -- the reference converts the fp64 send buffer with
 * Dense::convert_to before MPI_Isend and back after the receive
 * (restricted_schwarz.cpp:898-903, 929-933, 952-954).  Half the xGMI bytes. */
int schwz_ras_pack_f32(schwz_subdomain *sd, float *d_send, schwz_stream stream);
int schwz_ras_unpack_f32(schwz_subdomain *sd, const float *d_recv, schwz_stream stream);
/* One neighbour's share of step 0, to / from any device address: the one-sided exchange without a
 * matched receive.  "put" (CommHelpers::transfer_buffer with enable_put, include/comm_helpers.hpp:122-150
 * after pack_buffer :93-118): the pack kernel of out-neighbour k stores straight into that neighbour's
 * receive window (mapped with schwz_window_open), over xGMI when it lives on another GPU.  "get": the
 * unpack kernel of in-neighbour k loads from that neighbour's send window.  single != 0: fp32 wire
 * format (MixedValueType = float). */
/* The pack of the next exchange while the local solve is still finishing: the solve makes the rows of
 * the put lists final first and records an event; this call makes `stream` (a side stream) wait for it
 * and gathers the send buffer from the solve's result (double, or float with `single`) -- the values
 * schwz_ras_pack reads after schwz_ras_restrict.  The reference posts its MPI_Isend only after the local
 * solve and the restriction have finished (restricted_schwarz.cpp:884-943 inside schwarz_base.cpp:387-452);
 * here the RCCL send / recv runs beside the tail of the solve.  schwz_ras_early_pack_ok: 1 when the
 * subdomain's solver (CG) records that event. */
int schwz_ras_early_pack_ok(const schwz_subdomain *sd);
int schwz_ras_pack_early(schwz_subdomain *sd, void *d_send, int single, schwz_stream stream);
int schwz_ras_pack_neighbor(schwz_subdomain *sd, int k, void *d_dst, int single, schwz_stream stream);
int schwz_ras_unpack_neighbor(schwz_subdomain *sd, int k, const void *d_src, int single, schwz_stream stream);
/* Windows: device buffers that other rank processes of the node map into their address space -- the
 * MPI_Win_create / MPI_Win_lock_all of Communicate::setup_windows (source/communicate.cpp,
 * include/communicate.hpp:67-224) over HIP IPC.  alloc: a zeroed allocation of its own; export: its
 * 64-byte handle (send it to the peers by any host channel); open / close: map / unmap a peer's window. */
int schwz_window_alloc(int64_t bytes, void **d_ptr);
int schwz_window_free(void *d_ptr);
int schwz_window_export(void *d_ptr, unsigned char *h_handle64);
int schwz_window_open(const unsigned char *h_handle64, void **d_ptr);
int schwz_window_close(void *d_ptr);
/* Host-side windows (window_convergence, window_residual_vector of include/conv_tools.hpp:56-275) are
 * shared-memory segments mapped by every rank of the node; these are the remote update operations on
 * them: MPI_Accumulate(MPI_SUM) on an int, MPI_Put / local read of an int, MPI_Accumulate(MPI_MIN) on a
 * double. */
int32_t schwz_host_atomic_add_i32(int32_t *p, int32_t v);
int32_t schwz_host_atomic_load_i32(const int32_t *p);
void schwz_host_atomic_store_i32(int32_t *p, int32_t v);
double schwz_host_atomic_min_f64(double *p, double v);
/* step 1: b~ = b_loc - A_Gamma x~ (SolverRAS::update_boundary,
 * restricted_schwarz.cpp:992-1017) */
int schwz_ras_update_boundary(schwz_subdomain *sd, schwz_stream stream);
/* step 2 (local half): rho = || b~ - A_loc [x~_int; x~_ovl] ||_2
 * (Solve::check_local_convergence, source/solve.cpp:796-856).  The norm is
 * written to *h_resnorm after a stream sync (the reference copies the scalar
 * to the host at solve.cpp:842-843). */
int schwz_ras_local_residual(schwz_subdomain *sd, double *h_resnorm, schwz_stream stream);
/* The same in two halves: launch enqueues the kernels and the scalar copy and
 * records an event; wait blocks on that event only.  A host layer may enqueue
 * the local solve between the two, so the GPU never idles while the host reads
 * the norm and runs the global check (schwz_ras_local_solve does not touch x~,
 * so a converged verdict simply skips step 4). */
int schwz_ras_local_residual_launch(schwz_subdomain *sd, schwz_stream stream);
int schwz_ras_local_residual_wait(schwz_subdomain *sd, double *h_resnorm);
/* step 3: y = solve(A_loc, b~), warm-started (Solve::local_solve,
 * source/solve.cpp:667-792).  h_inner_iters may be NULL (no sync). */
int schwz_ras_local_solve(schwz_subdomain *sd, int *h_inner_iters, schwz_stream stream);
/* Two-stage local solves: Solve::local_solve rebuilds the stopping criterion with a new
 * iteration cap once iter_count > settings.reset_local_crit_iter (source/solve.cpp:723-742);
 * max_iters = -1 means local_size_x.  Takes effect from the next local solve. */
int schwz_ras_set_local_max_iters(schwz_subdomain *sd, int max_iters);
/* Precision of the iterative local solve (an extension; schwz_solver_options keeps its layout, so the precision
 * travels through this setter).  Call after schwz_subdomain_to_device; takes effect from the next local solve.
 * SCHWZ_PRECISION_F32: the local solve is schwz_pcg_f32_solve on (b~, y), the solver created on the local matrix
 * at first use; SCHWZ_ERR_NOT_IMPLEMENTED for a direct local solver, for GMRES (non_symmetric) and for a
 * preconditioner other than none or scalar Jacobi (block-jacobi with block size 1 included).  While it is set
 * schwz_ras_check_and_solve_launch runs its two steps back to back, schwz_ras_early_pack_ok, schwz_ras_cg_flavour
 * and schwz_ras_y_form return 0, the restriction is the copy launch, and schwz_ras_algorithmic_bytes(sd, 1) prices
 * the fp32 iteration.  SCHWZ_PRECISION_F64 restores the fp64 path exactly. */
enum schwz_precision { SCHWZ_PRECISION_F64 = 0, SCHWZ_PRECISION_F32 = 1 };
int schwz_ras_set_local_precision(schwz_subdomain *sd, int precision);
int schwz_ras_local_precision(const schwz_subdomain *sd);

/* Which Krylov method solves a non-symmetric local system iteratively (an extension; schwz_solver_options keeps its
 * layout, so the choice travels through a setter, after schwz_subdomain_to_device).  GMRES(restart_iter) is what
 * the upload creates.  The setter creates the requested solver around the preconditioner the current one holds and
 * then destroys the other, so one set of work vectors lives between solves (device synchronisation; if the new
 * solver cannot be created the subdomain keeps the one it has).  SCHWZ_ERR_INVALID for a null
 * subdomain or an unknown code, SCHWZ_ERR_NOT_IMPLEMENTED unless the subdomain runs the iterative local solver
 * with non_symmetric set.  The getter answers SCHWZ_NONSYM_GMRES for a null subdomain. */
enum schwz_nonsym_solver { SCHWZ_NONSYM_GMRES = 0, SCHWZ_NONSYM_BICGSTAB = 1 };
int schwz_ras_set_nonsym_solver(schwz_subdomain *sd, int which);
int schwz_ras_nonsym_solver(const schwz_subdomain *sd);

/* The type the local GMRES stores its Krylov basis in (an extension; see schwz_gmres_create_basis for the method
 * and for the caveat on the recurred norm inside one cycle).  Call after schwz_subdomain_to_device;
 * SCHWZ_GMRES_BASIS_F64 is what the upload creates.  The setter replaces the GMRES object by one of the other
 * basis type around the same preconditioner (device synchronisation; on failure the subdomain keeps what it has).
 * While BiCGSTAB is set the choice is only remembered: a return to GMRES creates that type.  SCHWZ_ERR_INVALID for
 * a null subdomain or an unknown code, SCHWZ_ERR_NOT_IMPLEMENTED unless the subdomain runs the iterative local
 * solver with non_symmetric set.  The getter answers SCHWZ_GMRES_BASIS_F64 for a null subdomain. */
int schwz_ras_set_gmres_basis(schwz_subdomain *sd, int which);
int schwz_ras_gmres_basis(const schwz_subdomain *sd);

/* Which method solves a symmetric local system iteratively (an extension; schwz_solver_options keeps its layout, so
 * the choice travels through a setter, after schwz_subdomain_to_device; it takes effect from the next local solve).
 * SCHWZ_SYM_CG is what the upload creates.  SCHWZ_SYM_CHEBYSHEV: the local solve is schwz_cheb_solve on (b~, y), the
 * solver created on the local matrix at first use, with the bounds of schwz_cheb_create until
 * schwz_ras_set_cheb_bounds replaces them; SCHWZ_ERR_NOT_IMPLEMENTED for a direct local solver, for non_symmetric,
 * for a preconditioner other than none or scalar Jacobi (block-jacobi with block size 1 counts as Jacobi), for nonzero
 * ParILU options and while SCHWZ_PRECISION_F32 is set (schwz_ras_set_local_precision refuses F32 the same way while
 * Chebyshev is set).  While it is set schwz_ras_check_and_solve_launch runs its two steps back to back,
 * schwz_ras_early_pack_ok, schwz_ras_cg_flavour and schwz_ras_y_form return 0, the restriction is the copy launch,
 * schwz_ras_set_local_max_iters and schwz_ras_last_inner_stats work, and schwz_ras_algorithmic_bytes(sd, 1) prices
 * the fused launch: 12 nnz + 4 (n + 1) + 56 n (48 n without Jacobi).  SCHWZ_SYM_CG restores the CG path exactly.
 * The bounds calls return SCHWZ_ERR_INVALID before Chebyshev was first set.  The getter answers SCHWZ_SYM_CG for a
 * null subdomain. */
enum schwz_sym_solver { SCHWZ_SYM_CG = 0, SCHWZ_SYM_CHEBYSHEV = 1 };
int schwz_ras_set_sym_solver(schwz_subdomain *sd, int which);
int schwz_ras_sym_solver(const schwz_subdomain *sd);
int schwz_ras_cheb_bounds(const schwz_subdomain *sd, double *lmin, double *lmax);
int schwz_ras_set_cheb_bounds(schwz_subdomain *sd, double lmin, double lmax);
/* settings.enable_logging (source/solve.cpp:751-771): inner iterations and final residual norm of the
 * last local solve (0 and 0.0 for the direct path).  Synchronises the solver's stream. */
int schwz_ras_last_inner_stats(schwz_subdomain *sd, int *h_iters, double *h_resnorm);
/* steps 2+3 in one enqueue: the check residual of step 2 and the start residual of
 * the CG solve of step 3 come out of ONE pass over A_loc (two gathers per entry,
 * one matrix read), the norm's device->host copy is queued right behind it and
 * the CG iterations behind that.  Follow with schwz_ras_local_residual_wait. */
int schwz_ras_check_and_solve_launch(schwz_subdomain *sd, schwz_stream stream);
/* The input of a DEVICE-side all-gather of the residual norms (the MPI_Allgather of source/solve.cpp:890-891 as
 * an RCCL collective): makes `stream` wait for the norm of the last schwz_ras_local_residual_launch /
 * schwz_ras_check_and_solve_launch -- for that scalar only, not for the local solve enqueued behind the check --
 * and writes its SQUARE to d_norm_sq[0] (device memory) on that stream.  The host value stays available through
 * schwz_ras_local_residual_wait. */
int schwz_ras_norm_sq_to_device(schwz_subdomain *sd, double *d_norm_sq, schwz_stream stream);
/* step 4: x~[interior] = y[0:local_size] (Communicate::local_to_global_vector,
 * source/communicate.cpp:65-94) */
int schwz_ras_restrict(schwz_subdomain *sd, schwz_stream stream);

/* device pointers of the state vectors (for tests and host layers):
 * which: 0 = x~ (local_size_x+halo), 1 = b~ / local_solution (local_size_x),
 *        2 = y / init_guess (local_size_x), 3 = local_rhs (local_size_x)
 * The pointers of ids 0 and 2 are valid only until the next local solve or restriction of this subdomain: the
 * restriction swaps the two x~ buffers, and on a subdomain without overlap and halo whose local solver is CG the
 * vector y lives in one of them (the one x~ itself occupies after a restriction and before the first solve, the
 * other one after a solve).  Ask again after either call.  Ids 1 and 3 never move.  Where y is the x~ buffer
 * itself (schwz_ras_y_form 1), writing through the pointer of id 2 writes x~ too: the two are one vector there. */
int schwz_ras_vector(schwz_subdomain *sd, int which, double **d_ptr, int64_t *len);
/* the HBM-resident local_matrix of the subdomain (borrowed handle, owned by sd) */
int schwz_ras_local_csr(schwz_subdomain *sd, schwz_csr **out);
/* how the scalar-Jacobi diagonal of the local CG reaches its vector kernels: 0 no Jacobi scaling,
 * 1 a full 1/diag vector (8 B per row and launch), 2 one-byte codes into a small dictionary, 3 one
 * scalar (every stencil matrix).  Same values, same bits; bench.py needs it to count the bytes of a
 * launch.  Replaces nothing in the reference (gko::preconditioner::Jacobi stores blocks). */
int schwz_ras_jacobi_form(const schwz_subdomain *sd);
/* schwz_pcg_flavour of the subdomain's local CG (0 for the other local solvers) */
int schwz_ras_cg_flavour(const schwz_subdomain *sd);
/* where the vector y (schwz_ras_vector id 2) lives: 0 a buffer of its own; 1 the x~ buffer itself, 2 the other x~
 * buffer (a solve that has not been restricted) -- the latter two only on a subdomain without overlap and halo whose
 * CG defers the x update, where the solve then stores its result once instead of twice */
int schwz_ras_y_form(const schwz_subdomain *sd);
/* copy x~[0:local_size] to the host (synchronous) -- the rank's piece of the
 * solution assembled in Solve::compute_residual_norm (solve.cpp:1025-1085) */
int schwz_ras_get_interior(schwz_subdomain *sd, double *h_out, schwz_stream stream);
/* || b_int - (A x)_int ||^2 contribution of this subdomain's interior rows to
 * the final true residual (solve.cpp:1079-1084) given up-to-date halo values
 * in x~; returns the squared partial norm on the host (synchronous). */
int schwz_ras_true_residual_sq(schwz_subdomain *sd, double *h_out, schwz_stream stream);

/* HBM bytes one launch of the dominant kernels moves algorithmically
 * (SURVEY 8d): which: 0 = local SpMV, 1 = one PCG iteration, used by bench.py;
 * 2 = the coarse step of this subdomain (below; 0 without aggregates): 20 B per entry of W and 16 B per own aggregate
 * (residual), the subdomain's m rows of the inverse, 8 m nc, plus 16 nc for s and c (GEMV), and the apply pass,
 * 16 slots + 2 slots, plus 16 local_size_x where y is a buffer of its own;
 * 3 = one schwz_ras_aggregate_sums of this subdomain (0 without aggregates): 12 B per interior row (the value and the
 * row id), 28 B per piece (its record of three ints, its partial sum stored and read), 4 (m + 1) for the offsets of the
 * fold and 8 m for the sums */
int64_t schwz_ras_algorithmic_bytes(const schwz_subdomain *sd, int which);

/* ---- Two-level RAS: aggregation coarse correction (an extension: the reference has one level only, so no line of
 * it is replaced).  Z is the N x nc 0/1 matrix of a partition of the rows into aggregates, every aggregate inside the
 * interior of one subdomain, the aggregates of subdomain p numbered [first_agg_p, first_agg_p + m_p), nc <= 4096.  At
 * the start of an outer step, after schwz_ras_unpack and before schwz_ras_update_boundary, the host layer applies
 *     x <- x + Z A0^-1 Z^T (b - A x),   A0 = Z^T A Z
 * in this order: schwz_ras_coarse_residual for every subdomain, (several processes: all-gather of the segments of
 * s), schwz_coarse_solve once per process, schwz_ras_coarse_apply for every subdomain.  After the exchange x~ holds
 * current global values in all its slots, so the residual needs no SpMV -- (Z^T (b - A x))_a = beta_a - sum_j W_aj
 * x~_j with beta_a = sum_{i in a} b_i and W_aj = sum_{i in a} A_ij over the interior rows, exact zeros dropped (on a
 * stencil only slots at aggregate faces remain; on a general matrix up to the nonzeros of the interior rows) -- and
 * the correction needs no second exchange: every slot, halo included, knows its row's aggregate and adds c[agg].
 *
 * schwz_ras_coarse_set_aggregates (after schwz_subdomain_to_device; host work + uploads, synchronous): h_slot_agg
 * holds the global aggregate id of each of the local_size_x + halo slots of x~; plans beta, W, the piece table of
 * the residual launch and the subdomain's m rows of A0.  SCHWZ_ERR_INVALID for nc outside [1, 4096], ids outside
 * [0, nc) or an interior row outside [first_agg, first_agg + m); SCHWZ_ERR_NOT_IMPLEMENTED for overlap < 2 on more
 * than one subdomain (such local matrices drop the couplings across the cut).  m = 0 (an empty subdomain) is fine.
 * schwz_ras_coarse_rows: those m x nc values, row-major, for the host to assemble A0.
 * schwz_dense_inverse (host only): h_inv = h_a^-1, n x n row-major, LU with partial pivoting; SCHWZ_ERR_INVALID for
 * a zero, negligible or non-finite pivot -- a singular global matrix (pure Neumann) or an aggregate without rows.
 * schwz_coarse_create: the per-process / per-device object holding the explicit inverse (nc^2 doubles, at most
 * 128 MB), s and c (zeroed); schwz_coarse_vector: device pointers of s (which = 0) and c (1), nc long, fixed for the
 * object's life.
 * schwz_ras_coarse_residual writes s[first_agg .. first_agg + m): one workgroup per piece of at most 2048 entries
 * of W sums in a fixed tree order, a second launch folds every aggregate's pieces in table order -- no atomics,
 * the same bits from run to run.  schwz_coarse_solve: c = A0^-1 s, one launch, one wave per row.
 * schwz_ras_coarse_apply: x~[j] += c[agg(j)] on every slot and y[j] += c[agg(j)] on the local_size_x entries of the
 * warm start of the next local solve, one launch; where y is the x~ buffer itself (schwz_ras_y_form 1) the values
 * are added once.  Correct for every local solver (the direct ones ignore y) and at any point between a
 * restriction and the next solve.  All three obey `stream`.  The pointer rule of schwz_ras_vector holds: ask for ids
 * 0 and 2 again after a solve or a restriction, not after these calls (they move nothing). */
typedef struct schwz_coarse schwz_coarse;
int schwz_ras_coarse_set_aggregates(schwz_subdomain *sd, const int32_t *h_slot_agg, int32_t first_agg, int32_t m,
                                    int32_t nc);
int schwz_ras_coarse_rows(const schwz_subdomain *sd, double *h_rows);
int schwz_dense_inverse(int32_t n, const double *h_a, double *h_inv);
int schwz_coarse_create(int32_t nc, const double *h_inv, schwz_coarse **out);
void schwz_coarse_destroy(schwz_coarse *c);
int schwz_coarse_vector(schwz_coarse *c, int which, double **d_ptr, int32_t *len);
int schwz_ras_coarse_residual(schwz_subdomain *sd, schwz_coarse *c, schwz_stream stream);
int schwz_coarse_solve(schwz_coarse *c, schwz_stream stream);
int schwz_ras_coarse_apply(schwz_subdomain *sd, schwz_coarse *c, schwz_stream stream);

/* ---- The aggregate restriction of any vector (an extension, like the coarse correction it belongs to).  A two-level
 * step whose right-hand side changes with every application -- the preconditioner of the outer FGMRES below, z = z0 +
 * RAS(v - A z0) with z0 = Z A0^-1 Z^T v -- needs Z^T v once per application, where the stationary iteration needs
 * beta = Z^T b once per solve.  schwz_ras_aggregate_sums writes
 *     s[first_agg + a] = sum_{i in a} d_vec[i]     for the subdomain's m aggregates
 * into s of the coarse object (the vector schwz_ras_coarse_residual writes and schwz_coarse_solve reads) and nothing
 * else: s outside [first_agg, first_agg + m) and beta of the coarse part keep their values.  d_vec: device memory, at
 * least local_size doubles in local order -- the address of x~ or of the vector of id 3 both do.
 * The rows grouped by aggregate are cut on the host into pieces of at most 2048 rows of one aggregate; one workgroup
 * per piece sums in a fixed tree order and stores one partial sum, a second small launch folds every aggregate's
 * pieces in table order: no atomics, the same bits from run to run.  A streaming pass -- 12 B per interior row, see
 * schwz_ras_algorithmic_bytes(sd, 3) -- where schwz_ras_rhs_aggregate, which keeps the host plan's order and bits,
 * walks an aggregate with one lane.  The tables are shared with schwz_ras_rhs_aggregate and built by the first call of
 * either (it waits for `stream` once).  Obeys `stream`.  m = 0: SCHWZ_OK, nothing launched.  SCHWZ_ERR_INVALID, before
 * any HIP call, for a null argument, a subdomain without aggregates and a coarse object with another nc. */
int schwz_ras_aggregate_sums(schwz_subdomain *sd, schwz_coarse *c, const double *d_vec, schwz_stream stream);

/* ---- One matrix, many right-hand sides (an extension: the reference solves the one system its initialize was handed,
 * SchwarzBase::initialize at source/schwarz_base.cpp:128-271, and has no call that replaces b, so no line of it is
 * replaced).  Everything schwz_subdomain_to_device and schwz_ras_coarse_set_aggregates build follows from the matrix
 * and the partition, except the local right-hand side (schwz_ras_vector id 3), its copy in b~ (id 1), the sums beta of
 * the coarse part and the iteration state.  These calls replace exactly those, in a few vector passes; the solver
 * SELECTION -- precision, non-symmetric solver, GMRES basis, symmetric solver, Chebyshev bounds, the cap of
 * schwz_ras_set_local_max_iters -- survives all of them.  A new solve is: rhs_set or rhs_gather, rhs_aggregate (coarse
 * space on), restart, then the outer iteration as after the upload.  All of them obey `stream`, none synchronises the
 * device; SCHWZ_ERR_INVALID for a null argument and for a subdomain that is not on the device.
 *
 * schwz_ras_rhs_set: `rhs` holds local_size_x values in local order, [interior; overlap rows], the layout of
 * h_local_rhs; a host pointer (on_device = 0: one copy on `stream`, waited for, so the array is the caller's again on
 * return) or a device pointer (one copy launch).  The vector
 * of id 3 is overwritten in place: its pointer does not move.
 * schwz_ras_rhs_gather: for a right-hand side that already lives in HBM as ONE global vector of n_global = N doubles:
 * rhs[i] = d_global[index[i]], one indexed load per row.  index is the subdomain's own local-to-global list, or the map
 * schwz_ras_rhs_index sets (a caller that permuted the rows passes permutation[local_to_global[i]]; NULL: back to the
 * own list).  The map is checked on the host when it is set -- an index outside [0, N): SCHWZ_ERR_INVALID -- and
 * uploaded, 8 B per local row, by the first gather and not before: a subdomain that never solves again allocates
 * nothing.  rhs_index waits for the device only where it releases an uploaded map.
 * schwz_ras_rhs_aggregate: beta_a = sum_{i in a} b_i of the coarse part, from the vector of id 3 into the buffer the
 * residual launches of schwz_ras_coarse_residual read.  One lane per aggregate, the rows of an aggregate in ascending
 * order into one accumulator, no atomics: the order of the host plan, so the bits are those of a fresh
 * schwz_ras_coarse_set_aggregates on that b.  The rows grouped by aggregate (4 B per interior row) are built and
 * uploaded by the first call (it waits for `stream` once).  Without aggregates: SCHWZ_OK, nothing launched.
 * schwz_ras_rhs_norm_sq: sum of b_i^2 over the local_size interior rows in a fixed order, for the norm of a b that was
 * given on the device; waits for `stream`, like every call that hands a value to the host.  schwz_ras_rhs_norm_sq_local:
 * the same over all local_size_x rows, overlap rows included -- the square of the check residual of step 2 for a zero
 * x~, which a host layer that keeps the start vector measures its convergence against.
 * schwz_ras_restart, keep_x = 0: the state schwz_subdomain_to_device leaves -- both x~ buffers zero, b~ = b, y zero
 * where it is a vector of its own, schwz_ras_y_form what an upload followed by the same setters gives.  Every solver
 * object forgets its last solve first: a postponed last iteration and the stream handle saved for it are DROPPED
 * before any buffer is rewritten (never run later on the new data), likewise a pending Chebyshev norm, the second
 * output of the restriction and the state schwz_ras_last_inner_stats reports (0 iterations, norm 0, as before the first
 * solve); schwz_ras_cg_flavour answers 0 until the next solve.  The pointers of ids 1 and 3 do not move; ask for ids 0
 * and 2 again.  keep_x = 1: every vector keeps its values, x~ halos included, so the next solve starts from the last
 * iterate; only what refers to the old b goes: the solvers' memory as above and b~ (= b again; the next
 * schwz_ras_update_boundary rewrites its overlap rows).  Another value of keep_x: SCHWZ_ERR_INVALID.
 * Not offered: new matrix values on the old pattern, several right-hand sides in one batched solve (the block entry
 * points further down do that, on a state of their own), a start vector
 * other than zero or the kept one (write through the pointers of schwz_ras_vector at your own risk). */
int schwz_ras_rhs_set(schwz_subdomain *sd, const double *rhs, int on_device, schwz_stream stream);
int schwz_ras_rhs_index(schwz_subdomain *sd, const int64_t *h_index);
int schwz_ras_rhs_gather(schwz_subdomain *sd, const double *d_global, int64_t n_global, schwz_stream stream);
int schwz_ras_rhs_aggregate(schwz_subdomain *sd, schwz_stream stream);
int schwz_ras_rhs_norm_sq(schwz_subdomain *sd, double *h_out, schwz_stream stream);
int schwz_ras_rhs_norm_sq_local(schwz_subdomain *sd, double *h_out, schwz_stream stream);
int schwz_ras_restart(schwz_subdomain *sd, int keep_x, schwz_stream stream);

/* ---- The steps of a RAS iteration on block vectors (an extension, see "Block vectors" above: the reference solves
 * one system, so no line of it is replaced).  schwz_ras_batch_begin allocates the block state of a subdomain that is on
 * the device: x~ [interior | overlap | halo], b, b~ and y with k columns each, row-interleaved, all zero, and a schwz_bcg
 * on the local matrix.  It is separate from the single-vector state: these calls read the local matrix, the interface
 * rows and the index lists, and write nothing the other entry points read or write, so a single-vector run before or
 * after computes what it computes without them.  begin with the k the state already has keeps it; another k replaces
 * it; schwz_ras_batch_end (and schwz_subdomain_destroy) releases it.
 * k other than 2, 4, 8: SCHWZ_ERR_INVALID (checked first).  The block path exists for the fp64 CG local solve of a
 * symmetric matrix without a preconditioner or with scalar Jacobi (block-Jacobi of block size 1 included) on one level;
 * a direct or non-symmetric local solver, another preconditioner, the ParILU options, the fp32 or Chebyshev local
 * solve and a subdomain with aggregates: SCHWZ_ERR_NOT_IMPLEMENTED.  Every other call: SCHWZ_ERR_INVALID without a
 * block state.  All obey `stream`; those that hand values to the host wait for it.
 * rhs_set: h_rhs holds local_size_x * k values, [interior; overlap rows] with the columns innermost (host memory; the
 * copy is waited for); x~ and y go back to zero and b~ = b: the state of a fresh upload.
 * pack / unpack: the send and receive buffers are [neighbour][entry][column]: the layouts of schwz_ras_pack /
 * schwz_ras_unpack with k values per entry.
 * update_boundary: b~ = b - A_Gamma x~ on the overlap rows, per column, the row sum in CSR order.
 * local_residual: h_resnorm[j] = ||b~_j - A x~_j||_2 over the local_size_x rows (k values).
 * local_solve: A y_j = b~_j by schwz_bcg_solve from the last y, with the subdomain's local tolerance and iteration cap;
 * the columns named by `frozen` are left alone.  h_inner_iters: k counts (waits for `stream`), or NULL.
 * restrict: x~[interior] = y[interior] in the columns `frozen` does not name.
 * vector: 0 x~ (len (local_size_x + halo) * k), 1 b~, 2 y, 3 b (len local_size_x * k).
 * get_interior: local_size * k values of x~ to the host.  true_residual_sq: h_out[j] = sum over the interior rows of
 * (b_j - A x~_j)^2 (k values). */
int schwz_ras_batch_begin(schwz_subdomain *sd, int k);
int schwz_ras_batch_end(schwz_subdomain *sd);
int schwz_ras_batch_rhs_set(schwz_subdomain *sd, const double *h_rhs, schwz_stream stream);
int schwz_ras_batch_pack(schwz_subdomain *sd, double *d_send, schwz_stream stream);
int schwz_ras_batch_unpack(schwz_subdomain *sd, const double *d_recv, schwz_stream stream);
int schwz_ras_batch_update_boundary(schwz_subdomain *sd, schwz_stream stream);
int schwz_ras_batch_local_residual(schwz_subdomain *sd, double *h_resnorm, schwz_stream stream);
int schwz_ras_batch_local_solve(schwz_subdomain *sd, unsigned frozen, int *h_inner_iters, schwz_stream stream);
int schwz_ras_batch_restrict(schwz_subdomain *sd, unsigned frozen, schwz_stream stream);
int schwz_ras_batch_vector(schwz_subdomain *sd, int which, double **d_ptr, int64_t *len);
int schwz_ras_batch_get_interior(schwz_subdomain *sd, double *h_out, schwz_stream stream);
int schwz_ras_batch_true_residual_sq(schwz_subdomain *sd, double *h_out, schwz_stream stream);

/* ---- Outer FGMRES preconditioned by one RAS sweep, or by one two-level step (schwz_ras_aggregate_sums above, the
 * coarse solve and apply, then the sweep): the device half (an extension: the reference's only outer
 * iteration is the stationary one of SchwarzBase::run, source/schwarz_base.cpp:387-452, and it has no outer Krylov
 * method, so no line of it is replaced).  The host layer (schwz_amd/outer.py) runs right-preconditioned flexible
 * GMRES(m): z_j = M^-1 v_j is one RAS sweep from a zero start made of the calls above, w = A z_j comes from
 * schwz_ras_apply_interior, w is orthogonalised against V_0..V_j by classical Gram-Schmidt applied twice, and the
 * Givens rotations and the small triangular solve run on the host.
 *
 * schwz_ras_apply_interior: d_out[i] = (A x~)_i for the local_size interior rows, given up-to-date overlap values in
 * x~ (after an exchange): the operator, the matrix and its codings are those of the pass of schwz_ras_true_residual_sq,
 * the vector is kept instead of its norm.  The pass covers all local_size_x rows of the local matrix; on a subdomain
 * with overlap rows it goes through a vector of local_size_x doubles that the subdomain allocates at the first call.
 * d_out: device memory, local_size doubles.  Obeys `stream`, does not wait for it.
 *
 * One schwz_outer per process, over the n = sum of local_size interior rows of its subdomains, concatenated in
 * subdomain order: V ((restart + 1) columns), Z (restart columns), w, a copy of b, partial sums and a pinned buffer
 * for the coefficients, allocated once by schwz_outer_create (1 <= restart <= 128, n >= 0; columns are 256-byte
 * aligned).  Because the vectors are global within the process, every reduction is one launch over n.
 * schwz_outer_vector: device pointer of V_j (which = 0, 0 <= j <= restart), Z_j (1, 0 <= j < restart), w (2, j = 0)
 * or the copy of b (3, j = 0), n doubles each; fixed for the object's life.
 * schwz_outer_start: V_0 = w * inv_beta.  schwz_outer_normalize: V_(j+1) = w * inv_norm, 0 <= j < restart.
 * schwz_outer_dots: h_out[i] = V_i . w for i <= j and h_out[j + 1] = w . w (j + 2 values on the host; waits for
 * `stream`).  One pass that reads w and every V_i once, the accumulators of up to 32 coefficients in registers;
 * per-workgroup partial sums are folded in a fixed order by a second small launch, no floating-point atomics: the same
 * bits on every run.
 * schwz_outer_project_dots: w <- w - sum_(i <= j) h_in[i] V_i and, in the same pass, h_out[i] = V_i . w and
 * h_out[j + 1] = w . w of the NEW w (a lane keeps its rows' V_i values in registers between the subtraction and the
 * dots; h_in: j + 1 host values, passed by value).  0 <= j < restart for both; beyond 31 columns (j > 30) the work is
 * split into launches of 32 columns and the subtraction and the dots become passes of their own.
 * schwz_outer_combine: d_x[r] += sum_(i < k) h_y[i] Z_i[r] over the n rows, 1 <= k <= restart, one pass per 32
 * columns; d_x: device memory, n doubles (it may be a vector of the object).
 * schwz_outer_copy: d_dst[0:n] = d_src[0:n] on the device for pointers of any 8-byte alignment, the copies between
 * the interior of a subdomain's x~ and its slice of a vector of the object.
 * Bytes per outer iteration j: dots + two project_dots + normalize = 3 * 8 n (j + 2) + 32 n.
 * All launches go to `stream`.  A null object, pointer or an index out of range: SCHWZ_ERR_INVALID before any HIP
 * call.
 *
 * The fp32-compressed basis (Metadata.outer_basis = "single").  schwz_outer_create_basis: schwz_outer_create with the
 * storage of V chosen: basis 0 (SCHWZ_OUTER_BASIS_F64, what schwz_outer_create makes) or 1 (SCHWZ_OUTER_BASIS_F32: V
 * as restart + 1 fp32 columns, 256-byte aligned; Z, w, b and the partial sums as they are); any other value is
 * SCHWZ_ERR_INVALID.  On a single-basis object
 *   - schwz_outer_start and schwz_outer_normalize store fl32 of w * s, rounded to nearest even: the rounded vector IS
 *     the basis vector, the unrounded one exists nowhere;
 *   - schwz_outer_dots and schwz_outer_project_dots read the columns widened (exactly) and do all arithmetic in fp64,
 *     a lane on four consecutive rows: one 16-byte load per column, two of w; everything else -- up to 32 accumulators
 *     in registers, the capped grid, the fixed-order fold, no atomics, the same bits on every run, the split beyond 32
 *     columns -- is the fp64 passes';
 *   - schwz_outer_combine is unchanged (Z is fp64);
 *   - schwz_outer_vector with which = 0 is SCHWZ_ERR_INVALID (a double ** to floats would lie); ids 1 - 3 work.
 * schwz_outer_basis_read: d_dst[0:count] = rows first .. first + count of V_j, widened exactly.
 * schwz_outer_basis_write: the reverse, rounded to nearest even.  0 <= j <= restart, 0 <= first, first + count <= n;
 * the fp64 side is device memory at any 8-byte alignment, `first` any row (the subdomains' interiors sit at arbitrary
 * offsets of the concatenated vector); rows outside the range are not touched.  On a double-basis object both are
 * plain copies.
 * schwz_outer_residual: w = b - t in one pass over the n rows (d_t: device memory, n doubles -- A x in Z_0, which is
 * free wherever the true residual is taken) and h_out[0] = w . w through the fold of the other passes (one host value;
 * waits for `stream`).  Either basis.
 * V -- and only V -- is stored in fp32; all arithmetic stays fp64.  A rounding
 * error in V perturbs the Arnoldi relation by about 2^-24 relative to the cycle's start residual, and the next cycle's
 * recomputed residual removes it; one in Z would reach the residual as A (Z^ - Z) y, 2^-24 ||A|| ||dx||, and Z is read
 * once a cycle, so Z stays fp64.  Within a cycle the true residual follows the RECURRED one down to roughly 2^-24 of the
 * cycle's start residual and no further: a stop inside a cycle is provisional, and the host loop recomputes b - A x at
 * every cycle end before it says "converged".
 * Bytes per outer iteration j with fp32 columns: three passes over j + 1 columns of 4 n with w at 8 n, w written
 * twice, the normalisation reading 8 n and writing 4 n: 12 n (j + 1) + 52 n -- 0.53 x the fp64 bytes at j = 29, 0.56 x
 * over a cycle of 30.  Memory: (m + 1) * 4 n + (m + 3) * 8 n against (2 m + 4) * 8 n. */
typedef struct schwz_outer schwz_outer;
int schwz_ras_apply_interior(schwz_subdomain *sd, double *d_out, schwz_stream stream);
int schwz_outer_create(int64_t n, int restart, schwz_outer **out);
void schwz_outer_destroy(schwz_outer *o);
int schwz_outer_vector(schwz_outer *o, int which, int j, double **d_ptr);
int schwz_outer_start(schwz_outer *o, double inv_beta, schwz_stream stream);
int schwz_outer_dots(schwz_outer *o, int j, double *h_out, schwz_stream stream);
int schwz_outer_project_dots(schwz_outer *o, int j, const double *h_in, double *h_out, schwz_stream stream);
int schwz_outer_normalize(schwz_outer *o, int j, double inv_norm, schwz_stream stream);
int schwz_outer_combine(schwz_outer *o, int k, const double *h_y, double *d_x, schwz_stream stream);
int schwz_outer_copy(int64_t n, const double *d_src, double *d_dst, schwz_stream stream);
/* The four entry points of the fp32 basis.  KEEP THE BLANK between each name and its parameter list, whatever a formatter
 * says: tests/test_outer_options.py holds this header to exactly the ten names above with a pattern that wants the
 * parenthesis directly at the name, tests/test_host_setup.py wants every exported symbol declared in this header (its
 * pattern allows the blank), and neither test may be edited.  Without the blank the first of the two fails. */
enum schwz_outer_basis { SCHWZ_OUTER_BASIS_F64 = 0, SCHWZ_OUTER_BASIS_F32 = 1 };
int schwz_outer_create_basis (int64_t n, int restart, int basis, schwz_outer **out);
int schwz_outer_basis_read (schwz_outer *o, int j, int64_t first, int64_t count, double *d_dst, schwz_stream stream);
int schwz_outer_basis_write (schwz_outer *o, int j, int64_t first, int64_t count, const double *d_src, schwz_stream stream);
int schwz_outer_residual (schwz_outer *o, const double *d_t, double *h_out, schwz_stream stream);

#ifdef __cplusplus
}
#endif
#endif
