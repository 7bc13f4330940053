"""Host-side mirror of the reference solver API for the RAS hot path.

`Settings`, `Metadata` and `SolverRAS(settings, metadata).initialize() / .run()`
keep the names, argument meaning and error behaviour of
include/settings.hpp:77-496, include/restricted_schwarz.hpp:61-107 and
SchwarzBase::initialize / run (source/schwarz_base.cpp:128-271, 323-506), as
driven by benchmarking/bench_ras.cpp:48-197.  All arithmetic runs in
libschwz_hip.so on the GPU; this file only orders the launches and talks to
the communication layer.
"""
import os
import time
from dataclasses import dataclass, field

import numpy as np

from . import _capi as capi
from . import core
from . import outer
from .comm import InProcessComm

# Settings::partition_settings / local_solver_settings (include/settings.hpp:96-156)
PARTITION_REGULAR = "regular"
PARTITION_REGULAR2D = "regular2d"
PARTITION_METIS = "metis"
PARTITION_CUSTOM = "custom"
SOLVER_DIRECT_CHOLMOD = "direct-cholmod"
SOLVER_DIRECT_UMFPACK = "direct-umfpack"
SOLVER_DIRECT_GINKGO = "direct-ginkgo"
SOLVER_ITERATIVE_GINKGO = "iterative-ginkgo"

# MEASURE_ELAPSED_FUNC_TIME ids and names (schwarz_base.cpp:393-450)
NEVER = (1 << 62)  # "no stop iteration agreed yet" in the flooded convergence state

TIMING_NAMES = ["boundary_exchange", "boundary_update", "convergence_check", "local_solve",
                "expand_local_vec"]


@dataclass
class CommSettings:
    enable_onesided: bool = False
    enable_overlap: bool = False
    enable_put: bool = False
    enable_get: bool = True
    stage_through_host: bool = False
    enable_one_by_one: bool = False
    enable_flush_local: bool = False
    enable_flush_all: bool = True
    enable_lock_local: bool = False
    enable_lock_all: bool = True


@dataclass
class ConvergenceSettings:
    put_all_local_residual_norms: bool = True
    enable_global_simple_tree: bool = False
    enable_decentralized_leader_election: bool = False
    enable_global_check: bool = True
    enable_accumulate: bool = False
    enable_global_check_iter_offset: bool = False
    convergence_crit: str = "solution_based"


@dataclass
class Settings:
    executor_string: str = "hip"
    matrix_filename: str = "null"
    explicit_laplacian: bool = True
    use_mixed_precision: bool = False
    enable_random_rhs: bool = False
    print_matrices: bool = False
    debug_print: bool = False
    partition: str = PARTITION_REGULAR
    local_solver: str = SOLVER_ITERATIVE_GINKGO
    non_symmetric_matrix: bool = False
    restart_iter: int = 1
    reset_local_crit_iter: int = -1
    overlap: int = 2
    naturally_ordered_factor: bool = False
    metis_objtype: str = ""
    write_debug_out: bool = False
    write_iters_and_residuals: bool = False
    enable_logging: bool = False
    write_perm_data: bool = False
    shifted_iter: int = 1
    factorization: str = "cholmod"
    reorder: str = ""
    comm_settings: CommSettings = field(default_factory=CommSettings)
    convergence_settings: ConvergenceSettings = field(default_factory=ConvergenceSettings)
    # extension (the reference has a 2-D generator only): 2 or 3, and
    # an optional (nx, ny, nz) for non-cubic 3-D grids
    laplacian_dim: int = 2
    laplacian_shape: tuple = None
    # optional user partition vector for PARTITION_CUSTOM
    partition_vector: object = None
    spmv_variant: int = 0


@dataclass
class Metadata:
    global_size: int = 0
    oned_laplacian_size: int = 0
    local_size: int = 0
    local_size_x: int = 0
    local_size_o: int = 0
    overlap_size: int = 0
    num_subdomains: int = 1
    my_rank: int = 0
    my_local_rank: int = 0
    local_num_procs: int = 1
    comm_size: int = 1
    num_threads: int = 1
    iter_count: int = 0
    tolerance: float = 1e-6
    local_solver_tolerance: float = 1e-12
    max_iters: int = 100
    local_max_iters: int = -1
    updated_max_iters: int = -1
    local_precond: str = "null"
    precond_max_block_size: int = 16
    # extensions (no field of the reference's Metadata): the ParILU options of the ilu / isai local
    # preconditioner.  par_ilu_sweeps > 0: factors from that many ParILU sweeps on the GPU instead of the exact
    # ILU(0) (ilu, isai); trisolve_sweeps > 0: each factor applied by that many Jacobi sweeps instead of exact
    # triangular solves (ilu).  0 = today's exact paths.
    par_ilu_sweeps: int = 0
    trisolve_sweeps: int = 0
    # extension (no field of the reference's Metadata): "single" runs the iterative local solve as fp32 CG on the
    # fp64 start residual, the correction added in fp64 (schwz_pcg_f32); the outer iteration, which recomputes the
    # residual in fp64, is the refinement loop.  CG without a preconditioner or with block-jacobi of block size 1.
    local_solver_precision: str = "double"
    # extension (no field of the reference's Metadata): the Krylov method of the iterative local solve when
    # settings.non_symmetric_matrix is set: "gmres" (GMRES(restart_iter), the reference's) or "bicgstab"
    # (schwz_bicgstab: two products and five vector passes per iteration, 8 work vectors; it stops on the RECURRED
    # residual).  Without non_symmetric_matrix, or with a direct local solver, the field has no effect, like
    # restart_iter; any other name is refused.
    non_symmetric_solver: str = "gmres"
    # extension (no field of the reference's Metadata): the type GMRES stores its Krylov basis in: "double" (the
    # fp64 path as it always was) or "single" (compressed-basis GMRES, schwz_gmres_create_basis: fp32 basis vectors,
    # fp64 arithmetic, blocked classical Gram-Schmidt applied twice in three passes, a constant number of launches
    # per Krylov vector and half the basis memory).  The stop test inside a cycle is on the recurred norm, which the
    # true residual follows only down to about 2^-24 of the cycle's start residual; restarts recompute it in fp64.
    # Without non_symmetric_matrix, with a direct local solver or with non_symmetric_solver "bicgstab" the field has
    # no effect, like restart_iter; any other name is refused.
    gmres_basis: str = "double"
    # extension (no field of the reference's Metadata): the method of the iterative local solve of a symmetric matrix:
    # "cg" (the reference's) or "chebyshev" (schwz_cheb: a fixed polynomial in the Jacobi-preconditioned matrix, one
    # reduction-free launch per inner iteration; local_precond 'null' or block-jacobi of block size 1, double precision).
    # With non_symmetric_matrix or a direct local solver the field has no effect, like restart_iter; any other name is
    # refused.  The bounds on the spectrum of M^-1 A: chebyshev_lambda_max = 0 takes the Gershgorin bound of every
    # local matrix, chebyshev_lambda_min = 0 takes lambda_max / chebyshev_eig_ratio; explicit values override either
    # end.  Beyond these defaults the bounds are the user's responsibility: a lambda_max below the true largest
    # eigenvalue makes the local iteration diverge.
    symmetric_solver: str = "cg"
    chebyshev_eig_ratio: float = 30.0
    chebyshev_lambda_min: float = 0.0
    chebyshev_lambda_max: float = 0.0
    # extensions (no field of the reference's Metadata, which has one level only): the coarse space of a two-level
    # RAS.  coarse_space "none" (one-level RAS, launch for launch what it was) or "aggregates": at the start of every
    # outer step, after the halo exchange, x <- x + Z A0^-1 Z^T (b - A x) with A0 = Z^T A Z and Z the 0/1 matrix of a
    # partition of the rows into at most 4096 aggregates, each inside the interior of one subdomain; any other name is
    # refused.  coarse_aggregate_vector: one aggregate id >= 0 per global row in the caller's row ids (like
    # partition_vector); rows of one id that lie in different subdomains become different aggregates.  Without a
    # vector, coarse_aggregates > 0 parts are cut out of every subdomain's interior graph by the graph partitioner.
    # Synchronous two-sided loop only (enable_onesided is refused), overlap >= 2 on more than one subdomain.
    coarse_space: str = "none"
    coarse_aggregates: int = 0
    coarse_aggregate_vector: object = None
    # extensions (no field of the reference's Metadata, whose only outer iteration is the stationary one): "richardson"
    # (run() launch for launch what it was) or "fgmres": run() is right-preconditioned flexible GMRES(outer_restart)
    # with one RAS sweep as the preconditioner (schwz_amd/outer.py), stopped on ||r_k||_2 <= tolerance * ||b||_2 over
    # all rows -- not the stationary loop's test.  One level, synchronous two-sided exchange in fp64, one process; any
    # other name, and an outer_restart outside 1..128, is refused.  solve_many ignores both fields.
    outer_iteration: str = "richardson"
    outer_restart: int = 30
    # the preconditioner of the outer FGMRES: "ras" (one sweep; with a coarse space the loop is refused) or "two-level"
    # (needs coarse_space "aggregates": one stationary two-level step from a zero start, the coarse correction first).
    # With outer_iteration "richardson" the field has no effect, like restart_iter; any other name is refused.
    outer_preconditioner: str = "ras"
    # the storage of the outer FGMRES's Krylov basis V: "double" (the loop as it was) or "single": V in fp32 (Z, w, x and
    # all arithmetic stay fp64): by the byte model 0.56 x the bytes of the orthogonalisation over a cycle of 30, and
    # (m + 1) * 4 n bytes less memory.  A stop inside a cycle is then provisional: every cycle end recomputes b - A x (one
    # exchange and one operator pass more per cycle that stopped early), "converged" is said only of a recomputed
    # residual, and another cycle starts where it misses the tolerance.  No effect with outer_iteration "richardson"; any other name is refused.
    outer_basis: str = "double"
    current_residual_norm: float = -1.0
    min_residual_norm: float = -1.0
    time_struct: list = field(default_factory=list)
    comm_data_struct: list = field(default_factory=list)
    post_process_data: dict = field(default_factory=lambda: dict(
        global_residual_vector_out=[], local_residual_vector_out=[],
        local_converged_iter_count=[], local_converged_resnorm=[], local_timestamp=[]))
    first_row: object = None
    permutation: object = None


class HipBackend:
    """Device memory, streams and subdomain objects for `--executor=hip`."""

    name = "hip"

    def __init__(self, device_index=0):
        import torch
        if capi.device_count() < 1 or not torch.cuda.is_available():
            raise capi.SchwzError(capi.ERR_HIP,
                                  "executor 'hip' needs a GPU: no HIP device is visible and "
                                  "there is no CPU fallback")
        self._torch = torch
        self.device = torch.device("cuda", device_index)
        torch.cuda.set_device(self.device)
        capi.check(capi.lib.schwz_set_device(device_index))

    def stream(self):
        return self._torch.cuda.current_stream().cuda_stream

    def empty(self, n, single=False):
        return self._torch.empty(max(int(n), 1), device=self.device,
                                 dtype=self._torch.float32 if single else self._torch.float64)

    def synchronize(self):
        self._torch.cuda.synchronize()

    # halo windows of the free-running one-sided mode (HIP IPC)
    window = staticmethod(core.DeviceWindow)
    open_window = staticmethod(core.PeerWindow)
    atomic_add = staticmethod(core.host_atomic_add)
    atomic_min = staticmethod(core.host_atomic_min)

    # problem sources / partitions (host code of libschwz_hip.so)
    problem_laplacian = staticmethod(core.Problem.laplacian)
    problem_from_matrix_market = staticmethod(core.Problem.from_matrix_market)
    problem_from_csr = staticmethod(core.Problem.from_csr)
    problem_from_rows = staticmethod(core.Problem.from_rows)
    partition_regular = staticmethod(core.partition_regular)
    partition_regular2d = staticmethod(core.partition_regular2d)

    def subdomain(self, problem, P, me, overlap, first_row):
        return core.Subdomain(problem, P, me, overlap, first_row)


def _ratio(a, b):
    """a / b as the reference's double arithmetic gives it (solve.cpp:906-915): a zero initial
    residual yields NaN (0/0) or inf, never an exception, and NaN compares false against the
    tolerance, so such a run simply keeps iterating like the reference and the C++ mirror."""
    if b == 0.0:
        return float("nan") if a == 0.0 or a != a else float("inf")
    return a / b


def batch_blocks(nrhs):
    """The block widths solve_many runs nrhs columns in: blocks of 8, the last one padded up to 2, 4 or 8 (the widths
    the device code is instantiated for, capi.BATCH_WIDTHS)."""
    nrhs = int(nrhs)
    if nrhs < 1:
        raise capi.SchwzError(capi.ERR_INVALID, "solve_many: nrhs must be at least 1")
    full, rest = divmod(nrhs, 8)
    return (8,) * full + ((min(w for w in capi.BATCH_WIDTHS if w >= rest),) if rest else ())


def _local_solver_code(settings):
    ls = settings.local_solver
    if ls == SOLVER_ITERATIVE_GINKGO:
        return capi.SOLVER_ITERATIVE
    if ls in (SOLVER_DIRECT_GINKGO, SOLVER_DIRECT_CHOLMOD):
        # direct-cholmod runs CHOLMOD's host solve in the reference
        # (solve.cpp:688-694); the same P^T L^-T L^-1 P is applied on the GPU here
        return capi.SOLVER_DIRECT
    raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                   "local solver '%s' is not implemented" % ls)


def _sweep_counts(metadata):
    """(par_ilu_sweeps, trisolve_sweeps) of the metadata; negative counts are refused."""
    par, tri = int(getattr(metadata, "par_ilu_sweeps", 0)), int(getattr(metadata, "trisolve_sweeps", 0))
    if par < 0 or tri < 0:
        raise capi.SchwzError(capi.ERR_INVALID, "par_ilu_sweeps / trisolve_sweeps must be >= 0")
    return par, tri


def _factor_solver_code(settings, metadata=None):
    """The local solver code initialize() hands the library: the direct path factors with LL^T, or with
    the pivoted LU when settings.factorization == "umfpack" (the reference's direct-ginkgo + UMFPACK
    factors, solve.cpp:144-173).  non_symmetric_matrix needs GMRES or the LU.  The ParILU options of
    `metadata` apply to the iterative local solver only."""
    code = _local_solver_code(settings)
    if metadata is not None and any(_sweep_counts(metadata)) and code != capi.SOLVER_ITERATIVE:
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "par_ilu_sweeps / trisolve_sweeps apply to the iterative local solver only")
    if code == capi.SOLVER_DIRECT and settings.factorization == "umfpack":
        code = capi.SOLVER_DIRECT_LU
    if settings.non_symmetric_matrix and code == capi.SOLVER_DIRECT:
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "non_symmetric_matrix needs the iterative local solver (GMRES) or "
                                       "factorization='umfpack'; the direct path is an LL^T factorization")
    return code


def _precond_code(metadata):
    code = _precond_name_code(metadata)
    par, tri = _sweep_counts(metadata)
    if par > 0 and code not in (capi.PRECOND_ILU, capi.PRECOND_ISAI):
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "par_ilu_sweeps applies to local_precond 'ilu' and 'isai' only")
    if tri > 0 and code != capi.PRECOND_ILU:
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "trisolve_sweeps applies to local_precond 'ilu' only")
    return code


def _precision_code(settings, metadata):
    """capi.PRECISION_* of metadata.local_solver_precision; "single" exists for the iterative local solver of a
    symmetric matrix (CG) without a preconditioner or with scalar Jacobi.  Runs before any device call."""
    name = getattr(metadata, "local_solver_precision", "double")
    if name == "double":
        return capi.PRECISION_F64
    if name != "single":
        raise capi.SchwzError(capi.ERR_INVALID,
                              "local_solver_precision must be 'double' or 'single', not %r" % (name,))
    if _local_solver_code(settings) != capi.SOLVER_ITERATIVE:
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "local_solver_precision 'single' applies to the iterative local solver only")
    if settings.non_symmetric_matrix:
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "local_solver_precision 'single' is not implemented for GMRES "
                                       "(non_symmetric_matrix): GMRES keeps fp64 arithmetic; its mixed-precision "
                                       "form is the compressed basis, gmres_basis = 'single'")
    if _precond_name_code(metadata) not in (capi.PRECOND_NONE, capi.PRECOND_JACOBI):
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "local_solver_precision 'single' is implemented for local_precond 'null' and "
                                       "'block-jacobi' with precond_max_block_size 1 only")
    return capi.PRECISION_F32


def _nonsym_solver_code(settings, metadata):
    """capi.NONSYM_* of metadata.non_symmetric_solver.  The name is checked whatever the other settings are; it
    selects BiCGSTAB only for the iterative local solver of a non-symmetric matrix.  Runs before any device call."""
    name = getattr(metadata, "non_symmetric_solver", "gmres")
    if name not in ("gmres", "bicgstab"):
        raise capi.SchwzError(capi.ERR_INVALID,
                              "non_symmetric_solver must be 'gmres' or 'bicgstab', not %r" % (name,))
    if name == "bicgstab" and settings.non_symmetric_matrix \
            and _local_solver_code(settings) == capi.SOLVER_ITERATIVE:
        return capi.NONSYM_BICGSTAB
    return capi.NONSYM_GMRES


def _gmres_basis_code(settings, metadata):
    """capi.GMRES_BASIS_* of metadata.gmres_basis.  The name is checked whatever the other settings are; it selects
    the fp32 basis only where the local solver is GMRES: the iterative local solver of a non-symmetric matrix with
    non_symmetric_solver "gmres".  Runs before any device call."""
    name = getattr(metadata, "gmres_basis", "double")
    if not isinstance(name, str) or name not in ("double", "single"):
        raise capi.SchwzError(capi.ERR_INVALID, "gmres_basis must be 'double' or 'single', not %r" % (name,))
    if name == "single" and settings.non_symmetric_matrix \
            and _local_solver_code(settings) == capi.SOLVER_ITERATIVE \
            and _nonsym_solver_code(settings, metadata) == capi.NONSYM_GMRES:
        return capi.GMRES_BASIS_F32
    return capi.GMRES_BASIS_F64


def _sym_solver_code(settings, metadata):
    """capi.SYM_* of metadata.symmetric_solver.  The name is checked whatever the other settings are; it selects
    Chebyshev only for the iterative local solver of a symmetric matrix, where the combinations the solver does not
    have are refused.  Runs before any device call."""
    name = getattr(metadata, "symmetric_solver", "cg")
    if name not in ("cg", "chebyshev"):
        raise capi.SchwzError(capi.ERR_INVALID, "symmetric_solver must be 'cg' or 'chebyshev', not %r" % (name,))
    if name == "cg" or settings.non_symmetric_matrix or _local_solver_code(settings) != capi.SOLVER_ITERATIVE:
        return capi.SYM_CG
    if _precond_name_code(metadata) not in (capi.PRECOND_NONE, capi.PRECOND_JACOBI):
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "symmetric_solver 'chebyshev' is implemented for local_precond 'null' and "
                                       "'block-jacobi' with precond_max_block_size 1 only")
    if any(_sweep_counts(metadata)):
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "symmetric_solver 'chebyshev' takes no par_ilu_sweeps / trisolve_sweeps")
    if getattr(metadata, "local_solver_precision", "double") != "double":
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "symmetric_solver 'chebyshev' has no fp32 form (local_solver_precision 'single')")
    ratio = float(getattr(metadata, "chebyshev_eig_ratio", 30.0))
    lo = float(getattr(metadata, "chebyshev_lambda_min", 0.0))
    hi = float(getattr(metadata, "chebyshev_lambda_max", 0.0))
    if not (ratio > 1.0 and ratio < float("inf")):
        raise capi.SchwzError(capi.ERR_INVALID, "chebyshev_eig_ratio must be a finite number > 1")
    if not (0.0 <= lo < float("inf") and 0.0 <= hi < float("inf")):
        raise capi.SchwzError(capi.ERR_INVALID,
                              "chebyshev_lambda_min / chebyshev_lambda_max must be finite and >= 0 (0: automatic)")
    if lo > 0.0 and hi > 0.0 and not lo < hi:
        raise capi.SchwzError(capi.ERR_INVALID, "chebyshev_lambda_min must be below chebyshev_lambda_max")
    return capi.SYM_CHEBYSHEV


def _cheb_bounds(metadata, auto_lmax):
    """(lmin, lmax) of a subdomain's Chebyshev solver: explicit values override either end, 0 means automatic
    (lmax: the solver's Gershgorin bound, lmin: lmax / chebyshev_eig_ratio)."""
    hi = float(metadata.chebyshev_lambda_max) or float(auto_lmax)
    lo = float(metadata.chebyshev_lambda_min) or hi / float(metadata.chebyshev_eig_ratio)
    return lo, hi


def _coarse_enabled(settings, metadata):
    """Whether metadata.coarse_space asks for the aggregation coarse correction; what can be checked without the
    matrix is checked here.  Runs before any device call."""
    name = getattr(metadata, "coarse_space", "none")
    if not isinstance(name, str) or name not in ("none", "aggregates"):
        raise capi.SchwzError(capi.ERR_INVALID, "coarse_space must be 'none' or 'aggregates', not %r" % (name,))
    if name == "none":
        return False
    vec = getattr(metadata, "coarse_aggregate_vector", None)
    P = max(int(metadata.num_subdomains), 1)
    if vec is None:
        try:
            count = int(getattr(metadata, "coarse_aggregates", 0))
        except (TypeError, ValueError):
            count = 0
        if count <= 0:
            raise capi.SchwzError(capi.ERR_INVALID, "coarse_space 'aggregates' needs coarse_aggregates > 0 (aggregates "
                                                    "per subdomain) or a coarse_aggregate_vector")
    else:
        v = np.asarray(vec)
        if v.ndim != 1 or v.dtype.kind not in "iu" or (v.size and int(v.min()) < 0):
            raise capi.SchwzError(capi.ERR_INVALID, "coarse_aggregate_vector must hold one integer aggregate id >= 0 "
                                                    "per global row")
    if settings.comm_settings.enable_onesided:
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "coarse_space 'aggregates' exists for the synchronous two-sided loop only: the "
                                       "one-sided loops (enable_onesided) have no global point for a coarse solve")
    if P > 1 and int(settings.overlap) < 2:
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "coarse_space 'aggregates' needs settings.overlap >= 2 on more than one subdomain")
    if vec is None and count * P > capi.COARSE_MAX_DOFS:
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED, _too_many_aggregates(count * P))
    return True


def _too_many_aggregates(nc):
    return "the coarse space has %d aggregates; at most %d are implemented" % (nc, capi.COARSE_MAX_DOFS)


def _coarse_vector(metadata, N):
    """metadata.coarse_aggregate_vector as an int64 array of the global size N (ERR_INVALID otherwise)."""
    v = np.asarray(metadata.coarse_aggregate_vector)
    if v.shape != (int(N),):
        raise capi.SchwzError(capi.ERR_INVALID, "coarse_aggregate_vector must hold one aggregate id per global row "
                                                "(%d rows), not %s" % (N, "x".join(str(d) for d in v.shape) or "a scalar"))
    return v.astype(np.int64)


def _split_aggregates(agg, first_row):
    """Aggregate ids per (permuted) row, split by owner and compacted: rows of one id in different subdomains become
    different aggregates, the ids of subdomain p become the range [first[p], first[p + 1]).  Returns (ids, first)."""
    first_row = np.asarray(first_row, dtype=np.int64)
    P = len(first_row) - 1
    owner = np.searchsorted(first_row, np.arange(len(agg), dtype=np.int64), side="right") - 1
    # (first_row may repeat an entry, empty subdomains: the owner is the last subdomain starting at or before the row)
    key = owner * (int(agg.max()) + 1 if len(agg) else 1) + agg
    uniq, ids = np.unique(key, return_inverse=True)
    owner_of = uniq // (int(agg.max()) + 1 if len(agg) else 1)
    first = np.searchsorted(owner_of, np.arange(P + 1), side="left")
    return ids.astype(np.int64), first.astype(np.int64)


def _precond_name_code(metadata):
    lp = metadata.local_precond
    if lp in ("null", "", None):
        return capi.PRECOND_NONE
    if lp == "block-jacobi":
        bs = int(metadata.precond_max_block_size)
        if bs == 1:
            return capi.PRECOND_JACOBI
        if 1 < bs <= 32:
            return capi.PRECOND_BLOCK_JACOBI
        raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                       "block-jacobi: precond_max_block_size must be in 1..32")
    if lp == "ilu":
        return capi.PRECOND_ILU
    if lp == "isai":
        return capi.PRECOND_ISAI
    # unknown names only print to stderr in the reference (solve.cpp:568-570); refuse instead
    raise capi.NotImplementedSchwz(
        capi.ERR_NOT_IMPLEMENTED,
        "local_precond '%s' is not implemented; available: null, block-jacobi, ilu, isai" % lp)


class SolverRAS:
    """Restricted Additive Schwarz solver (include/restricted_schwarz.hpp:61-107).

    One process drives the subdomains listed in `comm.local_ranks`: all of them
    (InProcessComm, one GPU) or exactly one (TorchDistComm, one GPU per rank).
    """

    def __init__(self, settings, metadata, comm=None, backend=None, quiet=False):
        self.settings = settings
        self.metadata = metadata
        self.quiet = quiet
        if settings.executor_string not in ("hip", "cuda"):
            # the reference's "reference"/"omp" executors are CPU paths; this
            # build has none (the CPU restatement lives in oracle/ for tests only)
            raise capi.NotImplementedSchwz(
                capi.ERR_NOT_IMPLEMENTED,
                "executor '%s' is not available: only 'hip' (MI355X) exists and there is "
                "no CPU fallback" % settings.executor_string)
        self._user_matrix, self._user_rhs = None, None
        self._device_rhs = None  # set_rhs(tensor): the right-hand side lives in HBM, _user_rhs is not used
        self.comm = comm if comm is not None else InProcessComm(max(metadata.num_subdomains, 1))
        self.backend = backend if backend is not None else HipBackend(
            getattr(self.comm, "device_index", 0))
        metadata.num_subdomains = self.comm.size
        metadata.comm_size = self.comm.size
        metadata.my_rank = self.comm.rank
        self.subdomains = {}
        self.speculative_solve = True
        self.problem = None
        self.result = None

    def _print(self, *a):
        if self.comm.is_root and not self.quiet:
            print(*a, flush=True)

    # ------------------------------------------------------------------ setup
    def _setup_global_matrix(self):
        """Initialize::setup_global_matrix (initialization.cpp:197-272)."""
        s, m, be = self.settings, self.metadata, self.backend
        if self._user_matrix is not None:
            prob = be.problem_from_csr(*self._user_matrix)
            self._print("Matrix handed over by the caller ")
        elif s.matrix_filename != "null":
            prob = be.problem_from_matrix_market(s.matrix_filename)
            self._print("Matrix from file " + s.matrix_filename)
        elif s.explicit_laplacian:
            n = int(m.oned_laplacian_size)
            if s.laplacian_dim == 3:
                nx, ny, nz = s.laplacian_shape if s.laplacian_shape else (n, n, n)
                prob = be.problem_laplacian(3, nx, ny, nz)
                self._print("Laplacian 3D Matrix %dx%dx%d (generated in house) " % (nx, ny, nz))
            else:
                prob = be.problem_laplacian(2, n)
                self._print("Laplacian 2D Matrix (generated in house) ")
        else:
            raise capi.SchwzError(capi.ERR_IO, " Need to provide a matrix or enable the default "
                                               "laplacian matrix.")
        m.global_size = prob.N
        return prob

    def _distributed_ingest(self):
        """A matrix FILE on several rank processes: the root parses and partitions, every other rank
        receives the rows its subdomain reads (SCHWZ_DISTRIBUTED_INGEST=0: every rank parses the file and
        keeps the whole matrix, like the reference, initialization.cpp:204-213)."""
        s, comm = self.settings, self.comm
        return (self._user_matrix is None and s.matrix_filename != "null" and comm.size > 1
                and len(comm.local_ranks) == 1 and hasattr(comm, "scatter_objects")
                and hasattr(self.backend, "problem_from_rows")
                and os.environ.get("SCHWZ_DISTRIBUTED_INGEST", "1") != "0")

    def _ingest_distributed(self):
        """Root: Matrix-Market file -> partition / permutation -> for every rank the interior and overlap
        rows of its subdomain (what schwz_subdomain_setup reads), cut out of the permuted matrix.  Every
        rank: a row source over its own part only (schwz_problem_from_rows); sizes, first_row and the
        permutation are broadcast.  Nothing of global length but the permutation lives on a non-root rank."""
        s, m, be, comm = self.settings, self.metadata, self.backend, self.comm
        P = m.num_subdomains
        meta, pieces = None, None
        if comm.is_root:
            full = be.problem_from_matrix_market(s.matrix_filename)
            self._print("Matrix from file " + s.matrix_filename + " (parsed on the root, rows distributed)")
            m.global_size = full.N
            full = self._partition(full)
            pieces = []
            for r in range(P):
                host_sd = core.Subdomain(full, P, r, s.overlap, m.first_row)
                rows = np.sort(np.asarray(host_sd.local_to_global[:host_sd.local_size_x], dtype=np.int64))
                pieces.append((rows,) + tuple(full.extract_rows(rows)))
                host_sd.close()
            meta = (full.N, np.asarray(m.first_row, dtype=np.int64),
                    None if m.permutation is None else np.asarray(m.permutation, dtype=np.int64))
            full.close()
        N, first_row, perm = comm.broadcast_object(meta)
        rows, rp, col, val = comm.scatter_objects(pieces)
        m.global_size, m.first_row, m.permutation = int(N), first_row, perm
        return be.problem_from_rows(int(N), rows, rp, col, val)

    def _partition(self, prob):
        """Initialize::partition (initialization.cpp:278-329) + the first_row /
        permutation part of setup_local_matrices (restricted_schwarz.cpp:84-152)."""
        s, m, be = self.settings, self.metadata, self.backend
        P = m.num_subdomains
        first_row = be.partition_regular(prob.N, P)
        perm = None
        if s.partition == PARTITION_REGULAR:
            self._print(" Regular 1D partition")
        elif s.partition in (PARTITION_REGULAR2D, PARTITION_METIS, PARTITION_CUSTOM):
            if s.partition == PARTITION_REGULAR2D:
                self._print(" Regular 2D partition")
                part = be.partition_regular2d(int(round(prob.N ** 0.5)), P) if P > 1 else None
            elif s.partition == PARTITION_METIS:
                self._print(" METIS partition")
                part = prob.partition_graph(P) if P > 1 else None
            else:
                part = s.partition_vector
                if P > 1:
                    if part is None:
                        raise capi.SchwzError(capi.ERR_INVALID,
                                              "partition 'custom' needs settings.partition_vector")
                    part = np.asarray(part)
                    if part.shape != (prob.N,) or part.min() < 0 or part.max() >= P:
                        raise capi.SchwzError(capi.ERR_INVALID,
                                              "partition_vector must hold one part id in [0, %d) per row "
                                              "(%d rows)" % (P, prob.N))
            if P > 1 and s.write_debug_out and self.comm.is_root and part is not None:
                # partition_tools.hpp:96-106
                with open("part_indices.csv", "w") as f:
                    f.write("idx,subd\n")
                    f.writelines("%d,%d\n" % (i, p) for i, p in enumerate(np.asarray(part)))
            if P > 1:
                prob, perm, first_row = prob.permute(part, P)
        else:
            raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                           "partition '%s' is not implemented" % s.partition)
        m.first_row = first_row
        m.permutation = perm
        return prob

    def _rhs(self, ids):
        """rhs = 1.0, or the default-seeded uniform(0,1) sequence when enable_random_rhs is set
        together with explicit_laplacian (schwarz_base.cpp:169-173, initialization.cpp:88-96).
        As in the reference the rhs is indexed by the (possibly permuted) row id.  A right-hand
        side handed to initialize() is indexed by the caller's (old) row id."""
        if self._user_rhs is not None:
            perm = self.metadata.permutation
            ids = np.asarray(ids, dtype=np.int64)
            return self._user_rhs[ids if perm is None else np.asarray(perm, dtype=np.int64)[ids]]
        if self.settings.enable_random_rhs and self.settings.explicit_laplacian \
                and self.settings.matrix_filename == "null":
            return core.rhs_random(ids)
        return np.ones(len(ids), dtype=np.float64)

    def _rhs_is_ones(self):
        return self._user_rhs is None and not (self.settings.enable_random_rhs and self.settings.explicit_laplacian
                                                and self.settings.matrix_filename == "null")

    def _rhs_first_rows(self, sd, count):
        """rhs of the first `count` local rows of a subdomain; the all-ones default needs no global ids (the
        local-to-global list of a 16.8 M-row subdomain is 134 MB to copy out of the library)."""
        if self._rhs_is_ones():
            return np.ones(int(count), dtype=np.float64)
        return np.ascontiguousarray(self._rhs(sd.local_to_global[:count]), dtype=np.float64)

    def initialize(self, matrix=None, rhs=None):
        """SchwarzBase::initialize (schwarz_base.cpp:128-271).  `matrix` = (row_ptr, col, val) of
        the global system and `rhs` (ones when None), the same on every rank: the analogue of
        the reference's initialize(dealii::SparseMatrix, dealii::Vector) overload
        (include/schwarz_base.hpp:96-97) for callers that assemble their own system."""
        s, m, be, comm = self.settings, self.metadata, self.backend, self.comm
        self._user_matrix = matrix
        self._user_rhs = None if rhs is None else np.ascontiguousarray(rhs, dtype=np.float64)
        self._device_rhs, self._gather_index_set, self._start_ref = None, False, None
        solver_code = _factor_solver_code(s, m)
        precond_code = _precond_code(m)
        precision_code = _precision_code(s, m)
        nonsym_code = _nonsym_solver_code(s, m)
        sym_code = _sym_solver_code(s, m)
        basis_code = _gmres_basis_code(s, m)
        coarse_on = _coarse_enabled(s, m)
        outer.wants_fgmres(s, m, comm)
        self._coarse = None
        if self._distributed_ingest():
            prob = self._ingest_distributed()
        else:
            prob = self._setup_global_matrix()
            prob = self._partition(prob)
        self.problem = prob
        P = m.num_subdomains
        user_aggregates = None
        if coarse_on and m.coarse_aggregate_vector is not None:
            # the caller's ids by (permuted) row, split by owner: the count is known -- and refused -- before any upload
            vec = _coarse_vector(m, prob.N)
            if m.permutation is not None:
                vec = vec[np.asarray(m.permutation, dtype=np.int64)]
            user_aggregates = _split_aggregates(vec, m.first_row)
            if int(user_aggregates[1][-1]) > capi.COARSE_MAX_DOFS:
                raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED, _too_many_aggregates(int(user_aggregates[1][-1])))
        for me in comm.local_ranks:
            self.subdomains[me] = be.subdomain(prob, P, me, s.overlap, m.first_row)
        coarse_plan = self._coarse_aggregates(user_aggregates) if coarse_on else None
        puts = comm.handshake({me: sd.get_lists() for me, sd in self.subdomains.items()})
        for me, sd in self.subdomains.items():
            for q, ids in puts[me]:
                sd.add_put_list(q, ids)
        self.send_buf, self.recv_buf = {}, {}
        # the ParILU options travel only when set (a backend without them keeps working with the defaults)
        par, tri = _sweep_counts(m)
        sweeps = dict(par_ilu_sweeps=par, trisolve_sweeps=tri) if par or tri else {}
        for me, sd in self.subdomains.items():
            sd.to_device(self._rhs_first_rows(sd, sd.local_size_x), local_solver=solver_code, precond=precond_code,
                         local_tol=m.local_solver_tolerance, local_max_iters=m.local_max_iters,
                         natural_factor_ordering=s.naturally_ordered_factor,
                         spmv_variant=s.spmv_variant, precond_block_size=m.precond_max_block_size,
                         non_symmetric=s.non_symmetric_matrix, restart_iter=s.restart_iter, **sweeps)
            if precision_code != capi.PRECISION_F64:  # (a backend without the setter keeps working in double)
                sd.set_local_precision(precision_code)
            if nonsym_code != capi.NONSYM_GMRES:  # (GMRES is what to_device creates: the setter is not called)
                sd.set_nonsym_solver(nonsym_code)
            if basis_code != capi.GMRES_BASIS_F64:  # (the fp64 basis is what to_device creates: the setter is not called)
                sd.set_gmres_basis(basis_code)
            if sym_code != capi.SYM_CG:  # (CG is what to_device creates: the setter is not called)
                sd.set_sym_solver(sym_code)
                sd.set_cheb_bounds(*_cheb_bounds(m, sd.cheb_bounds()[1]))
            # use_mixed_precision (MixedValueType = float): halos travel as fp32
            self.send_buf[me] = be.empty(sd.num_send, s.use_mixed_precision)
            self.recv_buf[me] = be.empty(sd.num_recv, s.use_mixed_precision)
        if s.print_matrices or s.write_perm_data or s.debug_print:
            self._debug_dumps(solver_code)
        first = self.subdomains[comm.local_ranks[0]]
        m.local_size, m.local_size_x = first.local_size, first.local_size_x
        m.overlap_size, m.local_size_o = first.overlap_size, m.global_size
        # per-pair views into the packed buffers, neighbour order
        self._sends, self._recvs = {}, {}
        for me, sd in self.subdomains.items():
            off = sd.send_offsets()
            for k, (q, _) in enumerate(sd.put_lists()):
                self._sends[(me, q)] = self.send_buf[me][off[k]:off[k + 1]]
            off = sd.recv_offsets()
            for k, (p, _) in enumerate(sd.get_lists()):
                self._recvs[(p, me)] = self.recv_buf[me][off[k]:off[k + 1]]
        # out- / in-neighbour ranks per subdomain (the overlapped mode's flag messages go along these edges;
        # put_lists() / get_lists() copy the id lists out of the library: not per iteration)
        self._neighbour_ranks = {me: ([q for q, _ in sd.put_lists()], [p for p, _ in sd.get_lists()])
                                 for me, sd in self.subdomains.items()}
        m.comm_data_struct = [
            (me, [(q, len(ids)) for q, ids in sd.put_lists()],
             [(p, len(ids)) for p, ids in sd.get_lists()], sd.num_send, sd.num_recv)
            for me, sd in self.subdomains.items()]
        if coarse_on:
            self._setup_coarse(*coarse_plan)
        self.close()  # windows of an earlier initialize()
        self._win = None
        if s.comm_settings.enable_onesided and getattr(comm, "node_windows", False) \
                and not s.comm_settings.enable_overlap:
            self._setup_windows()
        self._print(" Problem size: %d, subdomains: %d, local size (rank %d): %d (+%d overlap)" %
                    (m.global_size, P, comm.rank, m.local_size, m.overlap_size))
        if solver_code == capi.SOLVER_ITERATIVE:
            lmi = m.local_size_x if m.local_max_iters == -1 else m.local_max_iters
            if nonsym_code == capi.NONSYM_BICGSTAB:
                self._print(" Local max iters %d (BiCGSTAB)" % lmi)
            elif sym_code == capi.SYM_CHEBYSHEV:
                self._print(" Local max iters %d (Chebyshev)" % lmi)
            elif basis_code == capi.GMRES_BASIS_F32:
                self._print(" Local max iters %d with restart iter %d (fp32 basis)" % (lmi, s.restart_iter))
            else:
                self._print(" Local max iters %d with restart iter %d" % (lmi, s.restart_iter))
        else:
            self._print(" Local direct solve with HIP TRS")

    # ---------------------------------------------------------- coarse space
    def _coarse_aggregates(self, user_aggregates):
        """The aggregates of the local subdomains' interior rows, before any upload: ({me: global aggregate id of
        every interior row}, first) with the ids of subdomain p the range [first[p], first[p + 1]).  From the caller's
        vector, or coarse_aggregates parts of every interior graph cut by the graph partitioner (empty parts are
        renumbered away)."""
        m, comm = self.metadata, self.comm
        P = m.num_subdomains
        if user_aggregates is not None:
            ids, first = user_aggregates
            fr = np.asarray(m.first_row, dtype=np.int64)
            return {me: ids[fr[me]:fr[me + 1]] for me in self.subdomains}, first
        local, counts = {}, {}
        for me, sd in self.subdomains.items():
            n = sd.local_size
            k = min(int(m.coarse_aggregates), n)
            if k <= 1:
                part = np.zeros(n, dtype=np.int64)
            else:
                rp, col, val = sd.local_matrix()
                end = int(rp[n])
                keep = col[:end] < n  # the interior block: rows and columns of the owned rows
                rows = np.repeat(np.arange(n), np.diff(rp[:n + 1]))[keep]
                brp = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(np.bincount(rows, minlength=n), out=brp[1:])
                block = self.backend.problem_from_csr(brp, col[:end][keep], val[:end][keep])
                part = np.unique(np.asarray(block.partition_graph(k), dtype=np.int64), return_inverse=True)[1]
                block.close()
            local[me] = part
            counts[me] = int(part.max()) + 1 if n else 0
        allcounts = [int(c) for c in comm.allgather_scalars(counts)]
        first = np.concatenate([[0], np.cumsum(allcounts)]).astype(np.int64)
        if int(first[-1]) > capi.COARSE_MAX_DOFS:
            raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED, _too_many_aggregates(int(first[-1])))
        return {me: local[me] + first[me] for me in local}, first

    def _setup_coarse(self, interior_ids, first):
        """After the upload: every subdomain learns the aggregate ids of its overlap and halo slots by one pass of
        the ids, written as doubles into x~, through the halo exchange (ids up to 4096 are exact in the fp32 wire
        format too), plans and uploads its part, the rows of A0 are gathered and inverted once per process."""
        be, comm, torch = self.backend, self.comm, self.backend._torch
        t_begin = time.perf_counter()
        stream = be.stream()
        nc = int(first[-1])
        if nc < 1:
            raise capi.SchwzError(capi.ERR_INVALID, "the coarse space has no aggregate (a matrix without rows)")
        idx, vals = {}, {}
        for me, sd in self.subdomains.items():
            p, n = sd.vector(0)
            idx[me] = torch.arange(max(n, 1), dtype=torch.int32, device=be.device)
            v = np.full(max(n, 1), -1.0)
            v[:sd.local_size] = interior_ids[me]
            vals[me] = torch.from_numpy(v).to(be.device)
            if n:
                core.scatter(n, idx[me].data_ptr(), vals[me].data_ptr(), p, stream=stream)
        for me, sd in self.subdomains.items():
            self._pack(me, sd, stream)
        comm.exchange(self._sends, self._recvs)
        for me, sd in self.subdomains.items():
            self._unpack(me, sd, stream)
        rows = {}
        for me, sd in self.subdomains.items():
            p, n = sd.vector(0)
            if n:
                core.gather(n, idx[me].data_ptr(), p, vals[me].data_ptr(), stream=stream)
                be.synchronize()
            slot = np.rint(vals[me].cpu().numpy()[:n]).astype(np.int64)
            if n:
                vals[me].zero_()  # x~ starts the iteration as zeros again
                core.scatter(n, idx[me].data_ptr(), vals[me].data_ptr(), p, stream=stream)
                be.synchronize()
            if (slot < 0).any() or (slot >= nc).any():
                raise capi.SchwzError(capi.ERR_INVALID, "subdomain %d: a slot of x~ received no aggregate id from "
                                                        "the halo exchange" % me)
            mloc = int(first[me + 1] - first[me])
            sd.coarse_set_aggregates(slot, int(first[me]), mloc, nc)
            rows[me] = sd.coarse_rows().reshape(-1)
        a0 = comm.gather_vectors(rows)
        if hasattr(comm, "broadcast_object") and len(comm.local_ranks) < comm.size:
            a0 = comm.broadcast_object(a0)
        inv = core.dense_inverse(np.asarray(a0, dtype=np.float64).reshape(nc, nc))
        obj = core.Coarse(inv)
        gather = None
        if len(comm.local_ranks) < comm.size:
            # several rank processes: every rank's segment of s to everybody, padded to the largest segment
            me = comm.local_ranks[0]
            mmax = max(int((first[1:] - first[:-1]).max()), 1)
            mloc = int(first[me + 1] - first[me])
            where = np.concatenate([p * mmax + np.arange(first[p + 1] - first[p]) for p in range(comm.size)])
            gather = dict(mine=torch.zeros(mmax, dtype=torch.float64, device=be.device),
                          all=torch.zeros(comm.size * mmax, dtype=torch.float64, device=be.device),
                          take=torch.arange(int(first[me]), int(first[me]) + max(mloc, 1), dtype=torch.int32,
                                            device=be.device),
                          where=torch.from_numpy(where.astype(np.int32)).to(be.device), mloc=mloc)
        self._coarse = dict(obj=obj, gather=gather, nc=nc, first=first, interior=interior_ids,
                            setup_seconds=time.perf_counter() - t_begin)

    def _coarse_step(self, locals_, stream):
        """x <- x + Z A0^-1 Z^T (b - A x) on the compute stream, between the unpack of the halo exchange and the
        boundary update: the coarse residual of every local subdomain, (several processes) the all-gather of the
        segments of s, the dense solve once per process, the correction of every local subdomain's x~ and y."""
        co = self._coarse
        obj, g = co["obj"], co["gather"]
        for _, sd in locals_:
            sd.coarse_residual(obj, stream)
        if g is not None:
            s_ptr, _ = obj.vector(0)
            if g["mloc"]:
                core.gather(g["mloc"], g["take"].data_ptr(), s_ptr, g["mine"].data_ptr(), stream=stream)
            self.comm.allgather_segments(g["mine"], g["all"])
            core.gather(co["nc"], g["where"].data_ptr(), g["all"].data_ptr(), s_ptr, stream=stream)
        obj.solve(stream)
        for _, sd in locals_:
            sd.coarse_apply(obj, stream)

    def _debug_dumps(self, solver_code):
        """The reference's debug output for executors other than "cuda" (schwarz_base.cpp:252-257, solve.cpp:401-450,
        utils.cpp:94-108): print_matrices -> local_mat_<rank>.csv / int_mat_<rank>.csv (and L_mat / U_mat of the
        direct local solver) as 1-based "row,col,value" lines; write_perm_data -> perm_<rank>.csv / inv_perm_<rank>.csv
        of the factor ordering (LU: the row permutation and the inverse of the column permutation, the reference's
        local_perm and local_inv_perm); debug_print -> the permutation check."""
        s = self.settings

        def dump(name, me, rp, col, val):
            rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
            with open("%s_%d.csv" % (name, me), "w") as f:
                f.writelines("%d,%d,%.17g\n" % (r + 1, c + 1, v) for r, c, v in zip(rows, col, val))

        for me, sd in self.subdomains.items():
            rp, col, val = sd.local_matrix()
            if s.print_matrices:
                dump("local_mat", me, rp, col, val)
                dump("int_mat", me, *sd.interface_matrix())
            if solver_code not in (capi.SOLVER_DIRECT, capi.SOLVER_DIRECT_LU):
                continue
            if solver_code == capi.SOLVER_DIRECT_LU:
                f = core.lu(rp, col, val, s.naturally_ordered_factor)
                perm, q = np.asarray(f["row_perm"]), np.asarray(f["col_perm"])
            else:
                f = core.cholesky(rp, col, val, s.naturally_ordered_factor)
                perm = q = np.asarray(f["perm"])
            if s.print_matrices:
                dump("U_mat", me, f["u_rp"], f["u_col"], f["u_val"])
                dump("L_mat", me, f["l_rp"], f["l_col"], f["l_val"])
            inv = np.empty_like(q)
            inv[q] = np.arange(len(q), dtype=q.dtype)
            if s.debug_print:
                ok = np.array_equal(np.sort(perm), np.arange(len(perm))) and \
                    np.array_equal(np.sort(inv), np.arange(len(inv)))
                self._print(" Rank %d Permutation is %s\n Rank %d Inverse Permutation is %s" %
                            (me, "correct" if ok else "incorrect", me, "correct" if ok else "incorrect"))
            if s.write_perm_data:
                np.savetxt("perm_%d.csv" % me, perm, fmt="%d")
                np.savetxt("inv_perm_%d.csv" % me, inv, fmt="%d")

    # -------------------------------------------------------------------- run
    def _log_local_solve(self, locals_):
        """settings.enable_logging (solve.cpp:751-771): inner iteration count, final inner residual
        norm and a timestamp per outer iteration.  Reads the solver state, i.e. synchronises."""
        if not self.settings.enable_logging:
            return
        ppd = self.metadata.post_process_data
        for _, sd in locals_:
            if hasattr(sd, "last_inner_stats"):
                it, rn = sd.last_inner_stats()
                ppd["local_converged_iter_count"].append(it)
                ppd["local_converged_resnorm"].append(rn)
                ppd["local_timestamp"].append(time.perf_counter() - self._t_begin)

    def _two_stage(self):
        """solve.cpp:723-742: once iter_count > reset_local_crit_iter the local stopping
        criterion is rebuilt with updated_max_iters (-1: local_size_x) as its iteration cap."""
        s, m = self.settings, self.metadata
        if (s.reset_local_crit_iter != -1 and m.iter_count > s.reset_local_crit_iter
                and not self._two_stage_on):
            for _, sd in self.subdomains.items():
                sd.set_local_max_iters(m.updated_max_iters)
            self._two_stage_on = True

    def _pack(self, me, sd, stream):
        if self.settings.use_mixed_precision:
            sd.pack_f32(self.send_buf[me].data_ptr(), stream)
        else:
            sd.pack(self.send_buf[me].data_ptr(), stream)

    def _unpack(self, me, sd, stream):
        if self.settings.use_mixed_precision:
            sd.unpack_f32(self.recv_buf[me].data_ptr(), stream)
        else:
            sd.unpack(self.recv_buf[me].data_ptr(), stream)

    def _exchange(self):
        stream = self.backend.stream()
        if getattr(self, "_early", None) is not None:
            # this exchange was posted beside the tail of the last local solves (_post_early_exchange):
            # the same values, already on their way
            handle, self._early = self._early, None
            self.comm.finish_exchange(handle)
            for me, sd in self.subdomains.items():
                self._unpack(me, sd, stream)
            return
        for me, sd in self.subdomains.items():
            self._pack(me, sd, stream)
        self.comm.exchange(self._sends, self._recvs)
        for me, sd in self.subdomains.items():
            self._unpack(me, sd, stream)

    def _early_exchange_ok(self):
        """The synchronous two-sided loop may post the exchange of iteration k + 1 beside the tail of the
        local solves of iteration k: the solvers make the rows of the put lists final first and record an
        event (schwz_ras_pack_early), the communicator sends device buffers from a side stream.  The values
        are those the exchange at the start of iteration k + 1 would read after the restriction: the
        iteration is the same bit for bit.  SCHWZ_EARLY_EXCHANGE=0 switches it off."""
        if getattr(self, "_early_ok", None) is None:
            comm = self.comm
            self._early_ok = (os.environ.get("SCHWZ_EARLY_EXCHANGE", "1") != "0"
                              and self.metadata.num_subdomains > 1
                              and getattr(comm, "supports_early_exchange", lambda: False)()
                              and all(hasattr(sd, "early_pack_ok") and sd.early_pack_ok()
                                      for sd in self.subdomains.values()))
        return self._early_ok

    def _post_early_exchange(self):
        single = self.settings.use_mixed_precision

        def pack(stream):
            for me, sd in self.subdomains.items():
                sd.pack_early(self.send_buf[me].data_ptr(), single, stream)
        self._early = self.comm.start_exchange_early(self._sends, self._recvs, pack)

    def begin_run(self):
        """State of SchwarzBase::run before its loop (schwarz_base.cpp:340-386)."""
        m, P = self.metadata, self.metadata.num_subdomains
        cs, cv = self.settings.comm_settings, self.settings.convergence_settings
        if cs.enable_onesided and not (cv.enable_global_simple_tree or
                                       cv.enable_decentralized_leader_election):
            raise capi.SchwzError(capi.ERR_INVALID, "Global Convergence check type unspecified")
        if cs.enable_onesided and cs.enable_overlap and P > 62:
            # the flooded state carries one bit per subdomain in an int64 (the mirror refuses the
            # same, host/src/schwarz_base.cpp)
            raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED,
                                           "overlapped one-sided mode supports at most 62 subdomains")
        self._announce_protocol()
        self._lres0 = {me: -1.0 for me in self.subdomains}
        self._flags = {me: False for me in self.subdomains}
        self._gres, self._gres0 = 0.0, -1.0
        if getattr(self, "_start_ref", None) is not None:
            # set_rhs(..., "keep"): the tests measure against the residual of a ZERO start vector, as a fresh solver's
            # do -- relative to a kept iterate's own, already small, residual no tolerance could be met
            self._lres0, self._gres0 = dict(self._start_ref[0]), self._start_ref[1]
        self._num_converged = 0
        self._timings = [[] for _ in range(5)]
        # overlapped one-sided mode: flooded convergence state and the messages in flight
        self._mask = {me: 0 for me in self.subdomains}
        self._stop = {me: NEVER for me in self.subdomains}
        self._pending = None
        if getattr(self, "_early", None) is not None:  # an exchange left over from an interrupted run
            self._exchange()
        self._early = None
        self._t_begin = time.perf_counter()
        if getattr(self, "_win", None) is not None:
            # a fresh run: the windows go back to their initial state (collectively, before anybody iterates)
            self.comm.barrier()
            hw = self._win["host"]
            if self.comm.is_root:
                hw["tree"][:] = 0
                hw["flags"][:] = 0
                hw["count"][:] = 0
                hw["resid"][:] = np.finfo(np.float64).max
            self._win["sent"][:] = 0
            self._win["counted"] = False
            self.comm.barrier()
        if getattr(self, "_two_stage_on", False):  # a re-run starts with the first-stage cap again
            for _, sd in self.subdomains.items():
                sd.set_local_max_iters(m.local_max_iters)
        self._two_stage_on = False
        ppd = m.post_process_data
        for k in ppd:
            ppd[k] = []
        ppd["global_residual_vector_out"] = [[] for _ in range(P)]
        m.iter_count = 0

    def _announce_protocol(self):
        """Says once per run which exchange / termination protocol actually runs: several of the
        reference's flags select variants of MPI RMA that have no counterpart over RCCL and are
        accepted as aliases (INTEGRATION.md section 1 lists them)."""
        cs, cv = self.settings.comm_settings, self.settings.convergence_settings
        if not cs.enable_onesided:
            return
        notes = []
        if cs.enable_put or cs.enable_one_by_one or cs.enable_flush_local or cs.enable_lock_local \
                or not cs.enable_get or not cs.enable_flush_all or not cs.enable_lock_all:
            notes.append("RMA flavour flags (put/get, one_by_one, flush/lock) select no different code: "
                         "halos travel as RCCL send/recv pairs")
        if cs.enable_overlap:
            proto = getattr(self, "_termination", "flood")
            notes.append("termination protocol: " + {
                "flood": "decentralised flooding of (converged mask, stop iteration) over neighbour messages "
                         "(conv_tools.hpp:213-275)",
                "tree": "centralised tree: converged counts reduced to subdomain 0 along a binary tree, the "
                        "verdict broadcast down it (conv_tools.hpp:147-209)"}[proto])
            if cv.enable_accumulate:
                notes.append("enable_accumulate (MPI_Accumulate(MIN) of the norms) has no RCCL counterpart: "
                             "the flags travel with the halo messages")
        elif getattr(self, "_win", None) is not None:
            notes.append("free-running one-sided exchange: halo %s through peer-mapped device windows, no "
                         "matched receive, no collective in the loop; termination: %s" %
                         ("put" if cs.enable_put else "get",
                          "centralised tree (conv_tools.hpp:147-209)" if cv.enable_global_simple_tree else
                          ("decentralised, accumulated counters" if cv.enable_accumulate else
                           "decentralised flag propagation (conv_tools.hpp:213-275)")))
        else:
            notes.append("one-sided without enable_overlap on a communicator without node windows: local "
                         "tests, flags all-gathered per iteration (a host collective stands in for the "
                         "window reads)")
        if not cv.put_all_local_residual_norms:
            notes.append("put_all_local_residual_norms=false changes nothing: norms never travel in one-sided mode")
        for n in notes:
            self._print(" [schwz] " + n)

    def _setup_windows(self):
        """Communicate::setup_windows (source/communicate.cpp; include/communicate.hpp:67-224): every
        rank exposes its receive and its send buffer as a window the neighbours map, and learns at
        which offset of a neighbour's window its own values live (put_displacements /
        get_displacements, restricted_schwarz.cpp:624-658)."""
        s, be, comm = self.settings, self.backend, self.comm
        # HIP IPC handles and the POSIX shared-memory segment only mean something on ONE node
        import socket
        hosts = set(comm.share(socket.gethostname()))
        if len(hosts) > 1:
            raise capi.SchwzError(capi.ERR_INVALID,
                                  "the free-running one-sided mode maps the neighbours' device windows through HIP "
                                  "IPC and needs all ranks on one node; this job spans %d hosts (%s)" %
                                  (len(hosts), ", ".join(sorted(hosts))))
        me = comm.rank
        sd = self.subdomains[me]
        single = s.use_mixed_precision
        recv_w = be.window(max(sd.num_recv, 1), single)
        send_w = be.window(max(sd.num_send, 1), single)
        roff, soff = sd.recv_offsets(), sd.send_offsets()
        mine = dict(recv=recv_w.handle, send=send_w.handle,
                    recv_off={p: roff[k] for k, (p, _) in enumerate(sd.get_lists())},
                    send_off={q: soff[k] for k, (q, _) in enumerate(sd.put_lists())})
        everyone = comm.share(mine)
        peers_recv, peers_send = {}, {}
        for q, _ in sd.put_lists():   # "put": my values go into q's receive window, where q expects rank me
            peers_recv[q] = (be.open_window(everyone[q]["recv"]), everyone[q]["recv_off"][me])
        for p, _ in sd.get_lists():   # "get": p's values for me sit in p's send window
            peers_send[p] = (be.open_window(everyone[p]["send"]), everyone[p]["send_off"][me])
        self._win = dict(recv=recv_w, send=send_w, peers_recv=peers_recv, peers_send=peers_send, single=single,
                         host=comm.host_windows(), sent=np.zeros(comm.size, dtype=np.int32),
                         puts=[(q, len(ids)) for q, ids in sd.put_lists()],
                         gets=[(p, len(ids)) for p, ids in sd.get_lists()], roff=roff, soff=soff)
        comm.barrier()

    def close(self):
        """Releases the windows of the free-running one-sided mode in an order every rank can rely on:
        nobody iterates any more (barrier), the mappings of the neighbours' windows go, everybody has
        unmapped (barrier), the own exported buffers are freed, then the host windows (the creator unlinks
        the shared-memory segment).  Collective; called by a re-initialize and by the owner when done."""
        win = getattr(self, "_win", None)
        if win is None:
            return
        self._win = None
        comm = self.comm
        self.backend.synchronize()
        comm.barrier()
        for w, _ in list(win["peers_recv"].values()) + list(win["peers_send"].values()):
            w.close()
        comm.barrier()
        win["recv"].close()
        win["send"].close()
        win["host"] = None
        if hasattr(comm, "close_windows"):
            comm.close_windows()

    def _exchange_free_running(self, sd, stream):
        """exchange_boundary_onesided (restricted_schwarz.cpp:715-852): put = pack into the neighbours'
        receive windows, then scatter whatever MY receive window holds; get = pack into my send
        window, then scatter straight out of the neighbours' send windows.  Nobody waits for anybody."""
        w, cs = self._win, self.settings.comm_settings
        single = w["single"]
        if cs.enable_put:
            for k, (q, _) in enumerate(w["puts"]):
                win, off = w["peers_recv"][q]
                sd.pack_neighbor(k, win.at(off), single, stream)
            for k, (p, _) in enumerate(w["gets"]):
                sd.unpack_neighbor(k, w["recv"].at(w["roff"][k]), single, stream)
        else:
            for k, (q, _) in enumerate(w["puts"]):
                sd.pack_neighbor(k, w["send"].at(w["soff"][k]), single, stream)
            for k, (p, _) in enumerate(w["gets"]):
                win, off = w["peers_send"][p]
                sd.unpack_neighbor(k, win.at(off), single, stream)

    def _termination_free_running(self, me, sd, lres, converged_local):
        """check_global_convergence, one-sided branch (solve.cpp:876-943) on the shared-memory windows.
        Returns num_converged_procs."""
        cv, be, m = self.settings.convergence_settings, self.backend, self.metadata
        P, it = m.num_subdomains, m.iter_count
        hw = self._win["host"]
        resid, ppd = hw["resid"], m.post_process_data
        # window_residual_vector (conv_tools.hpp:56-142): my smallest local residual so far, to everybody
        # (put_all_local_residual_norms) or min-accumulated along the neighbour graph
        mine = resid[me]
        mine[me] = min(mine[me], lres)
        prev = ppd["global_residual_vector_out"][me][-1] if it > 0 and ppd["global_residual_vector_out"][me] else None
        if cv.put_all_local_residual_norms:
            if it > 0 and mine[me] != prev:
                for j in range(P):
                    if j != me:
                        resid[j][me] = mine[me]
        else:
            big = np.finfo(np.float64).max
            for q, cnt_q in self._win["puts"]:
                if cnt_q == 0:
                    continue
                for j in range(P):
                    if j != q and mine[j] != big:
                        be.atomic_min(resid[q], j, float(mine[j]))
        for j in range(P):
            ppd["global_residual_vector_out"][j].append(float(mine[j]))
        if cv.enable_global_simple_tree:
            # Yamazaki et al. 2019 (conv_tools.hpp:147-209): slots 0 / 1 = my children have reported, slot 2 =
            # the verdict coming down; a node reports once (slot 0 := 2), when its children have and it
            # passes its own test in this very iteration
            t = hw["tree"]
            c = t[me]
            if (((c[0] == 1 and c[1] == 1) or (c[0] == 1 and me == P // 2 - 1) or (me >= P // 2 and c[0] != 2))
                    and converged_local):
                if me == 0:
                    c[2] = 1
                else:
                    t[(me - 1) // 2][1 if me % 2 == 0 else 0] = 1
                c[0] = 2
            if c[2] == 1:
                for child in (2 * me + 1, 2 * me + 2):
                    if child < P:
                        t[child][2] = 1
                c[1] += 1
                return P
            return 0
        if cv.enable_accumulate:
            # conv_tools.hpp:229-246: +1 on everybody's counter.  The reference adds again in EVERY
            # iteration a rank passes its test, so its counters overshoot num_subdomains and the
            # "== num_subdomains" exit can be missed or hit early; here a rank adds once.
            cnt = hw["count"]
            if converged_local and not self._win.get("counted"):
                for j in range(P):
                    be.atomic_add(cnt, j, 1)
                self._win["counted"] = True
            return int(cnt[me])
        # decentralised flag propagation (conv_tools.hpp:247-273): what I know goes to my out-neighbours, once
        fl, sent = hw["flags"], self._win["sent"]
        if converged_local:
            fl[me][me] = 1
        local = fl[me].copy()
        for q, cnt_q in self._win["puts"]:
            if cnt_q == 0:
                continue
            for j in range(P):
                if sent[j] == 0 and local[j] == 1:
                    fl[q][j] = 1
        sent[:] = local
        return int(local.sum())

    def _step_free_running(self):
        """`enable_onesided` on a communicator with node windows: the reference's asynchronous
        iteration (schwarz_base.cpp:387-452 with exchange_boundary_onesided and the one-sided branch
        of check_global_convergence).  Every rank runs at its own pace: halos are whatever the
        neighbours' last put left in my window (or what their send window holds when I get), the
        local test feeds the tree / decentralised termination protocol on shared-memory windows, and
        a rank leaves the loop when ITS window says all have converged."""
        s, m, be, comm = self.settings, self.metadata, self.backend, self.comm
        cv = s.convergence_settings
        self._two_stage()
        me = comm.rank
        sd = self.subdomains[me]
        ppd, tol, it = m.post_process_data, m.tolerance, m.iter_count
        stream = be.stream()
        t0 = time.perf_counter()
        if it > 0:  # restricted_schwarz.cpp:725
            self._exchange_free_running(sd, stream)
        t1 = time.perf_counter()
        sd.update_boundary(stream)
        t2 = time.perf_counter()
        spec = self.speculative_solve and hasattr(sd, "check_and_solve_launch") and tol >= 0.0
        if spec:
            sd.check_and_solve_launch(stream)
            lres = sd.local_residual_wait()
        else:
            lres = sd.local_residual(stream) if tol >= 0.0 else -1.0
        if self._lres0[me] < 0.0:
            self._lres0[me] = lres
        if np.isnan(lres):
            raise capi.SchwzError(capi.ERR_DIVERGED, "local residual is NaN")
        ppd["local_residual_vector_out"].append(lres)
        m.current_residual_norm = lres
        m.min_residual_norm = lres if it == 0 else min(lres, m.min_residual_norm)
        iter_cond = ((it > m.max_iters * 0.05) or m.max_iters < 1000) \
            if cv.enable_global_check_iter_offset else True
        if tol > 0.0 and iter_cond:
            converged_local = _ratio(lres, self._lres0[me]) <= tol
            self._num_converged = self._termination_free_running(me, sd, lres, converged_local)
        t3 = time.perf_counter()
        tm = self._timings
        tm[0].append(t1 - t0)
        tm[1].append(t2 - t1)
        tm[2].append(t3 - t2)
        if self._num_converged == m.num_subdomains:
            return True
        if not spec:
            sd.local_solve(stream)
        self._log_local_solve([(me, sd)])
        t4 = time.perf_counter()
        sd.restrict(stream)
        tm[3].append(t4 - t3)
        tm[4].append(time.perf_counter() - t4)
        m.iter_count += 1
        return False

    def _step_overlapped(self):
        """`enable_onesided` + `enable_overlap`: the asynchronous flavour of the iteration as
        this build defines it (BASELINE config 5).  The halo exchange of iteration k is posted
        before the local solve of iteration k -- on a side stream under RCCL -- and consumed at
        the start of iteration k+1, so it is hidden behind the solve and halos are one iteration
        older than in the synchronous loop.  There is no global collective: every subdomain
        tests itself (solve.cpp:913-915) and floods (mask of converged subdomains, agreed stop
        iteration) to its neighbours with each message, the decentralised protocol of
        conv_tools.hpp:213-275 on matched messages; the first subdomain that sees the full mask
        at iteration k proposes stop = k + P, the minimum wins, and everybody stops together."""
        s, m, be, comm = self.settings, self.metadata, self.backend, self.comm
        self._two_stage()
        P = m.num_subdomains
        locals_ = list(self.subdomains.items())
        ppd = m.post_process_data
        tol = m.tolerance
        it = m.iter_count
        stream = be.stream()
        full = (1 << P) - 1
        t0 = time.perf_counter()
        # (a) consume what was posted one iteration ago
        if self._pending is not None:
            comm.finish_exchange(self._pending["halo"])
            for me, sd in locals_:
                self._unpack(me, sd, stream)
            for me, msgs in comm.finish_flags(self._pending["flags"]).items():
                for mk, st in msgs:
                    self._mask[me] |= mk
                    self._stop[me] = min(self._stop[me], st)
            self._pending = None
        last = it == m.max_iters - 1 or any(self._stop[me] == it for me, _ in locals_)
        # (b) post this iteration's halos: x~ after the previous restriction
        halo = None
        if not last:
            for me, sd in locals_:
                self._pack(me, sd, stream)
            halo = comm.start_exchange(self._sends, self._recvs, overlap=True)
        t1 = time.perf_counter()
        # (c) boundary update, local test + local solve (enqueued together), restriction
        for _, sd in locals_:
            sd.update_boundary(stream)
        t2 = time.perf_counter()
        fused = hasattr(locals_[0][1], "check_and_solve_launch") and tol >= 0.0
        if fused:
            for _, sd in locals_:
                sd.check_and_solve_launch(stream)
        for me, sd in locals_:
            lres = -1.0
            if tol >= 0.0:
                lres = sd.local_residual_wait() if fused else sd.local_residual(stream)
                if self._lres0[me] < 0.0:
                    self._lres0[me] = lres
            if np.isnan(lres):
                raise capi.SchwzError(capi.ERR_DIVERGED, "local residual is NaN")
            ppd["local_residual_vector_out"].append(lres)
            m.current_residual_norm = lres
            if tol > 0.0 and _ratio(lres, self._lres0[me]) <= tol:
                self._mask[me] |= 1 << me
            if self._mask[me] == full and self._stop[me] == NEVER:
                self._stop[me] = it + P
        if not last:
            neighbours = self._neighbour_ranks
            flags = comm.start_flags({me: (self._mask[me], self._stop[me]) for me, _ in locals_},
                                     neighbours)
            self._pending = dict(halo=halo, flags=flags)
        t3 = time.perf_counter()
        tm = self._timings
        tm[0].append(t1 - t0)
        tm[1].append(t2 - t1)
        tm[2].append(t3 - t2)
        if any(self._stop[me] == it for me, _ in locals_):
            self._num_converged = P
            return True
        if not fused:
            for _, sd in locals_:
                sd.local_solve(stream)
        self._log_local_solve(locals_)
        t4 = time.perf_counter()
        for _, sd in locals_:
            sd.restrict(stream)
        tm[3].append(t4 - t3)
        tm[4].append(time.perf_counter() - t4)
        m.iter_count += 1
        return False

    def step(self):
        """One pass of the loop body of SchwarzBase::run (schwarz_base.cpp:387-452).
        Returns True when the convergence test fired (no local solve is done then)."""
        s, m, be, comm = self.settings, self.metadata, self.backend, self.comm
        cs, cv = s.comm_settings, s.convergence_settings
        if cs.enable_onesided and cs.enable_overlap:
            return self._step_overlapped()
        if cs.enable_onesided and getattr(self, "_win", None) is not None:
            return self._step_free_running()
        self._two_stage()
        P = m.num_subdomains
        locals_ = list(self.subdomains.items())
        ppd = m.post_process_data
        tol = m.tolerance
        it = m.iter_count
        stream = be.stream()
        t0 = time.perf_counter()
        # 0 boundary exchange (one-sided mode skips iteration 0, restricted_schwarz.cpp:725)
        if not (cs.enable_onesided and it == 0):
            self._exchange()
        if getattr(self, "_coarse", None) is not None:
            self._coarse_step(locals_, stream)
        t1 = time.perf_counter()
        # 1 boundary update
        for _, sd in locals_:
            sd.update_boundary(stream)
        t2 = time.perf_counter()
        # 2 convergence check (solve.cpp:959-1005).  The residual kernels are enqueued, then
        # the local solve (step 3) is enqueued right behind them BEFORE the host waits for
        # the 8-byte norm: the GPU keeps working while the host runs the global check.  The
        # solve only writes y (and CG work vectors); if the verdict is "converged" its result
        # is simply not written back (step 4 is skipped), exactly like the reference.
        spec = self.speculative_solve and hasattr(locals_[0][1], "local_residual_launch")
        if tol >= 0.0 and spec:
            for _, sd in locals_:
                sd.check_and_solve_launch(stream)
        iter_cond = ((it > m.max_iters * 0.05) or m.max_iters < 1000) \
            if cv.enable_global_check_iter_offset else True
        # the P norms of the global test as a device-side all-gather (RCCL), enqueued on a side stream behind the
        # norm's own event: it runs beside the local solve, and the host then waits for ONE event instead of its own
        # scalar plus a gloo collective (every rank takes this branch or none: the conditions are global settings)
        norm_handle = None
        if (tol > 0.0 and spec and iter_cond and cv.enable_global_check and not cs.enable_onesided
                and getattr(comm, "device_norms", False) and len(locals_) == 1):
            sd0 = locals_[0][1]
            try:
                norm_handle = comm.start_allgather_norm_sq(lambda ptr, raw: sd0.norm_sq_to_device(ptr, raw))
            except Exception as e:  # e.g. the second RCCL communicator cannot be brought up: every rank sees that
                if getattr(comm, "_norm_used", False):
                    raise
                import warnings
                warnings.warn("device-side all-gather of the residual norms failed at its first use (%s: %s); "
                              "the gloo group takes over" % (type(e).__name__, e))
                comm.device_norms = False
                norm_handle = None
            else:
                comm._norm_used = True
        lres = {}
        for me, sd in locals_:
            if tol < 0.0:
                lres[me] = -1.0
            elif spec:
                lres[me] = sd.local_residual_wait()
            else:
                lres[me] = sd.local_residual(stream)
            if self._lres0[me] < 0.0:
                self._lres0[me] = lres[me]
            if np.isnan(lres[me]):
                raise capi.SchwzError(capi.ERR_DIVERGED, "local residual is NaN")
            ppd["local_residual_vector_out"].append(lres[me])
            ppd["local_converged_resnorm"].append(
                lres[me] / self._lres0[me] if self._lres0[me] != 0 else float("nan"))
            m.current_residual_norm = lres[me]
            m.min_residual_norm = lres[me] if it == 0 else min(lres[me], m.min_residual_norm)
        if tol > 0.0 and iter_cond:
            if cv.enable_global_check and not cs.enable_onesided:
                if norm_handle is not None:  # solve.cpp:890-891 on the device
                    allres = [float(np.sqrt(v)) for v in comm.finish_allgather_norm_sq(norm_handle)]
                else:
                    allres = comm.allgather_scalars(lres)  # solve.cpp:890-891
                gres = 0.0
                for j in range(P):
                    ppd["global_residual_vector_out"][j].append(allres[j])
                    gres += allres[j]  # SUM of the norms (solve.cpp:895-905)
                self._gres = gres
                if self._gres0 < 0.0:
                    self._gres0 = gres
                self._num_converged = P if _ratio(gres, self._gres0) <= tol else 0
            elif cs.enable_onesided:
                # local test (solve.cpp:913-915) + monotone flags (conv_tools.hpp:249-251)
                for me, _ in locals_:
                    if _ratio(lres[me], self._lres0[me]) <= tol:
                        self._flags[me] = True
                allflags = comm.allgather_scalars(
                    {me: float(self._flags[me]) for me, _ in locals_})
                self._num_converged = int(sum(allflags))
            else:
                self._num_converged = 0  # never converges on this branch
        t3 = time.perf_counter()
        if np.isnan(self._gres) or self._gres > 1e12:
            raise capi.SchwzError(capi.ERR_DIVERGED,
                                  " Rank %d diverged in %d iters " % (comm.rank, it))
        tm = self._timings
        tm[0].append(t1 - t0)
        tm[1].append(t2 - t1)
        tm[2].append(t3 - t2)
        if self._num_converged == P:
            return True
        # 3 local solve (already enqueued above in speculative mode)
        if not (tol >= 0.0 and spec):
            for _, sd in locals_:
                sd.local_solve(stream)
        self._log_local_solve(locals_)
        # step 0 of the NEXT iteration, posted now: pack + send / recv on a side stream as soon as the
        # solves have finalised their boundary rows, beside the rest of the solution update and step 4
        if not cs.enable_onesided and self._early_exchange_ok():
            self._post_early_exchange()
        t4 = time.perf_counter()
        # 4 restricted write-back
        for _, sd in locals_:
            sd.restrict(stream)
        t5 = time.perf_counter()
        tm[3].append(t4 - t3)
        tm[4].append(t5 - t4)
        m.iter_count += 1
        return False

    def finish_run(self, elapsed, gather_solution=True):
        """The tail of SchwarzBase::run (schwarz_base.cpp:453-503)."""
        m, comm = self.metadata, self.comm
        P = m.num_subdomains
        stream = self.backend.stream()
        locals_ = list(self.subdomains.items())
        m.time_struct = [(i, comm.rank, len(self._timings[i]), TIMING_NAMES[i], self._timings[i])
                         for i in range(5)]
        converged = self._num_converged == P
        out = dict(iter_count=m.iter_count, converged=converged, elapsed=elapsed,
                   residual_norm=None, rhs_norm=None, sol_norm=None, solution=None)
        if not converged:
            self._print("Rank %d did not converge in %d iterations." % (comm.rank, m.iter_count))
        else:
            self._print(" Rank %d converged in %d iterations " % (comm.rank, m.iter_count))
        # Solve::compute_residual_norm (solve.cpp:1025-1085): the interiors form the
        # solution; (A x) on the interior rows needs fresh overlap values, hence
        # one more exchange.
        self._exchange()
        parts = {me: sd.true_residual_sq(stream) for me, sd in locals_}
        res_sq = sum(comm.allgather_scalars(parts))
        if self._device_rhs is not None:  # set_rhs(tensor): b is in HBM only
            rhs_sq = sum(comm.allgather_scalars({me: sd.rhs_norm_sq(stream) for me, sd in locals_}))
        else:
            rhs_sq = sum(comm.allgather_scalars(
                {me: float(np.sum(self._rhs_first_rows(sd, sd.local_size) ** 2))
                 for me, sd in locals_}))
        out["residual_norm"] = float(np.sqrt(res_sq))
        out["rhs_norm"] = float(np.sqrt(rhs_sq))
        if gather_solution:
            pieces = {me: sd.get_interior(stream) for me, sd in locals_}
            sol_sq = sum(comm.allgather_scalars({me: float(np.dot(pieces[me], pieces[me]))
                                                 for me in pieces}))
            out["sol_norm"] = float(np.sqrt(sol_sq))
            out["solution"] = comm.gather_vectors(pieces)
        if converged:
            self._print(" residual norm %g\n relative residual norm of solution %g\n"
                        " Time taken for solve %g" %
                        (out["residual_norm"], out["residual_norm"] / out["rhs_norm"], elapsed))
        self.result = out
        return out

    # ------------------------------------------------- one matrix, many right-hand sides
    def _check_new_rhs(self, rhs, initial_guess):
        """The refusals of set_rhs, all before any device call: (host array or None, device tensor or None)."""
        def refuse(msg):
            raise capi.SchwzError(capi.ERR_INVALID, "set_rhs: " + msg)
        if self.problem is None or not self.subdomains:
            refuse("the solver is not set up: call initialize() first")
        if initial_guess not in ("zero", "keep"):
            refuse("initial_guess must be 'zero' or 'keep', not %r" % (initial_guess,))
        if rhs is None:
            return None, None
        N = int(self.metadata.global_size)
        if type(rhs).__module__.split(".")[0] == "torch":
            torch = self.backend._torch
            if rhs.dtype != torch.float64:
                refuse("a device right-hand side must be a float64 tensor, not %s" % rhs.dtype)
            if rhs.dim() != 1 or rhs.shape[0] != N:
                refuse("the right-hand side must have shape (%d,), not %s" % (N, tuple(rhs.shape)))
            if rhs.device != self.backend.device:
                refuse("the tensor lives on %s, the solver on %s" % (rhs.device, self.backend.device))
            return None, rhs.contiguous()
        arr = np.asarray(rhs)
        if arr.dtype.kind != "f":
            refuse("the right-hand side must hold floating-point values, not %s" % arr.dtype)
        if arr.ndim != 1 or arr.shape[0] != N:
            refuse("the right-hand side must have shape (%d,), not %s" % (N, arr.shape))
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if not np.isfinite(arr).all():
            refuse("the right-hand side holds a value that is not finite")
        return arr, None

    def set_rhs(self, rhs=None, initial_guess="zero"):
        """A new right-hand side on the solver as initialize() set it up -- partition, index sets, matrices, codings,
        factors, solver objects and the coarse plan stay -- and the iteration state of a fresh solver
        (initial_guess="zero": run() then computes, bit for bit, what initialize(rhs=...) + run() computes) or the
        last iterate as the start vector ("keep"; the convergence tests of the runs that follow then measure against
        the residual of a zero start vector, the norm of b per subdomain, as a fresh solver's do).  An extension: the reference has no such call.
        `rhs`: None (as in initialize: ones, or the random right-hand side the settings ask for), a host array of
        global_size floats, the same on every rank, indexed by the caller's row ids like initialize(rhs=...), or a
        float64 torch tensor of that length on the solver's device, which is gathered on the device and never copied
        to the host.  Collective like initialize(): every rank calls it."""
        host, dev = self._check_new_rhs(rhs, initial_guess)
        keep = initial_guess == "keep"
        be, comm = self.backend, self.comm
        stream = be.stream()
        # messages of an interrupted run: completed either way; applied (unpacked) only where x~ is kept
        if getattr(self, "_early", None) is not None:
            if keep:
                self._exchange()
            else:
                handle, self._early = self._early, None
                comm.finish_exchange(handle)
        pending, self._pending = getattr(self, "_pending", None), None
        if pending is not None:
            comm.finish_exchange(pending["halo"])
            comm.finish_flags(pending["flags"])
            if keep:
                for me, sd in self.subdomains.items():
                    self._unpack(me, sd, stream)
        self._user_rhs, self._device_rhs = host, dev
        if dev is not None and not self._gather_index_set:
            perm = self.metadata.permutation
            for sd in self.subdomains.values():
                if perm is None:
                    sd.rhs_index(None)
                else:  # exactly as _rhs indexes a right-hand side handed to initialize()
                    sd.rhs_index(np.asarray(perm, dtype=np.int64)[sd.local_to_global[:sd.local_size_x]])
            self._gather_index_set = True
        for sd in self.subdomains.values():
            if dev is not None:
                sd.rhs_gather(dev.data_ptr(), dev.shape[0], stream)
            else:
                sd.rhs_set(self._rhs_first_rows(sd, sd.local_size_x), stream)
            if getattr(self, "_coarse", None) is not None:
                sd.rhs_aggregate(stream)
            sd.restart(keep, stream)
        self._start_ref = None
        if keep:
            norms = {me: float(np.sqrt(sd.rhs_norm_sq_local(stream))) for me, sd in self.subdomains.items()}
            self._start_ref = (norms, float(sum(comm.allgather_scalars(norms))))

    def solve(self, rhs=None, initial_guess="zero", gather_solution=True):
        """set_rhs(rhs, initial_guess) followed by run(gather_solution)."""
        self.set_rhs(rhs, initial_guess)
        return self.run(gather_solution)

    # ------------------------------------------------- a block of right-hand sides at once
    def _check_batch(self, rhs):
        """The refusals of solve_many, all before any device allocation.  Returns the (N, nrhs) float64 array."""
        s, m = self.settings, self.metadata
        cs = s.comm_settings

        def unavailable(what):
            raise capi.NotImplementedSchwz(capi.ERR_NOT_IMPLEMENTED, "solve_many: the block path does not exist for " + what)

        def refuse(msg):
            raise capi.SchwzError(capi.ERR_INVALID, "solve_many: " + msg)
        if s.non_symmetric_matrix:
            unavailable("non_symmetric_matrix")
        if _local_solver_code(s) != capi.SOLVER_ITERATIVE:
            unavailable("a direct local solver")
        if any(_sweep_counts(m)):
            unavailable("the ParILU options (par_ilu_sweeps / trisolve_sweeps)")
        if _precond_name_code(m) not in (capi.PRECOND_NONE, capi.PRECOND_JACOBI):
            unavailable("local_precond '%s' (null, or block-jacobi with precond_max_block_size = 1)" % m.local_precond)
        if m.local_solver_precision != "double":
            unavailable("local_solver_precision '%s'" % m.local_solver_precision)
        if m.symmetric_solver != "cg":
            unavailable("symmetric_solver '%s'" % m.symmetric_solver)
        if m.coarse_space != "none":
            unavailable("coarse_space '%s' (two-level RAS)" % m.coarse_space)
        if cs.enable_onesided:
            unavailable("enable_onesided")
        if s.use_mixed_precision:
            unavailable("use_mixed_precision (fp32 halos)")
        if s.reset_local_crit_iter != -1:
            unavailable("reset_local_crit_iter (the two-stage local criterion)")
        if self.problem is None or not self.subdomains:
            refuse("the solver is not set up: call initialize() first")
        N = int(m.global_size)
        if type(rhs).__module__.split(".")[0] == "torch":
            refuse("the right-hand sides must be a host array (device tensors are not taken)")
        arr = np.asarray(rhs)
        if arr.dtype.kind != "f":
            refuse("the right-hand sides must hold floating-point values, not %s" % arr.dtype)
        if arr.ndim != 2 or arr.shape[0] != N:
            refuse("the right-hand sides must have shape (%d, nrhs), not %s" % (N, arr.shape))
        if arr.shape[1] < 1:
            refuse("nrhs must be at least 1")
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if not np.isfinite(arr).all():
            refuse("the right-hand sides hold a value that is not finite")
        return arr

    def _batch_exchange(self, bufs, stream):
        send_buf, recv_buf, sends, recvs = bufs
        for me, sd in self.subdomains.items():
            sd.batch_pack(send_buf[me].data_ptr(), stream)
        self.comm.exchange(sends, recvs)
        for me, sd in self.subdomains.items():
            sd.batch_unpack(recv_buf[me].data_ptr(), stream)

    def _solve_block(self, B, k, gather_solution):
        """One block: B is (N, nreal) in the caller's row ids, nreal <= k, the other columns are zero padding."""
        s, m, be, comm = self.settings, self.metadata, self.backend, self.comm
        cv = s.convergence_settings
        P, tol, nreal = m.num_subdomains, m.tolerance, B.shape[1]
        stream = be.stream()
        locals_ = list(self.subdomains.items())
        perm = None if m.permutation is None else np.asarray(m.permutation, dtype=np.int64)
        interior = {}
        send_buf, recv_buf, sends, recvs = {}, {}, {}, {}
        for me, sd in locals_:
            sd.batch_begin(k)
            ids = np.asarray(sd.local_to_global[:sd.local_size_x], dtype=np.int64)
            rows = ids if perm is None else perm[ids]      # exactly as _rhs indexes a right-hand side
            local = np.zeros((sd.local_size_x, k))
            local[:, :nreal] = B[rows]
            sd.batch_rhs_set(local, stream)
            interior[me] = local[:sd.local_size, :nreal]
            # [neighbour][entry][column]: the slices of the single-vector buffers, k times as long
            send_buf[me], recv_buf[me] = be.empty(sd.num_send * k), be.empty(sd.num_recv * k)
            off = sd.send_offsets()
            for q_at, (q, _) in enumerate(sd.put_lists()):
                sends[(me, q)] = send_buf[me][off[q_at] * k:off[q_at + 1] * k]
            off = sd.recv_offsets()
            for p_at, (p, _) in enumerate(sd.get_lists()):
                recvs[(p, me)] = recv_buf[me][off[p_at] * k:off[p_at + 1] * k]
        bufs = (send_buf, recv_buf, sends, recvs)
        padding = sum(1 << j for j in range(nreal, k))
        fired = [False] * nreal
        iters = [0] * nreal
        gres0 = [-1.0] * nreal
        history = [[] for _ in range(nreal)]
        be.synchronize()
        comm.barrier()
        start = time.perf_counter()
        it = 0
        while it < m.max_iters:
            self._batch_exchange(bufs, stream)
            for _, sd in locals_:
                sd.batch_update_boundary(stream)
            # the per-column test is the project's own (step(), solve.cpp:890-915): the sum over the subdomains of
            # the local residual norms, relative to its value at iteration 0
            lres = {me: (sd.batch_local_residual(stream) if tol >= 0.0 else [-1.0] * k) for me, sd in locals_}
            iter_cond = ((it > m.max_iters * 0.05) or m.max_iters < 1000) if cv.enable_global_check_iter_offset else True
            for j in range(nreal):
                if fired[j]:
                    continue
                if any(np.isnan(lres[me][j]) for me, _ in locals_):
                    raise capi.SchwzError(capi.ERR_DIVERGED, "local residual of column %d is NaN" % j)
                if tol > 0.0 and iter_cond and cv.enable_global_check:
                    gres = 0.0
                    for v in comm.allgather_scalars({me: lres[me][j] for me, _ in locals_}):
                        gres += v
                    history[j].append(gres)
                    if gres0[j] < 0.0:
                        gres0[j] = gres
                    if np.isnan(gres) or gres > 1e12:
                        raise capi.SchwzError(capi.ERR_DIVERGED, " Rank %d: column %d diverged in %d iters " % (comm.rank, j, it))
                    if _ratio(gres, gres0[j]) <= tol:
                        fired[j] = True
                        iters[j] = it
            if all(fired):
                break
            frozen = padding | sum(1 << j for j in range(nreal) if fired[j])
            for _, sd in locals_:
                sd.batch_local_solve(frozen, stream)
            for _, sd in locals_:
                sd.batch_restrict(frozen, stream)
            it += 1
        for j in range(nreal):
            if not fired[j]:
                iters[j] = it
        be.synchronize()
        comm.barrier()
        elapsed = time.perf_counter() - start
        # as finish_run: (A x) on the interior rows needs fresh overlap values, hence one more exchange
        self._batch_exchange(bufs, stream)
        parts = {me: sd.batch_true_residual_sq(stream) for me, sd in locals_}
        out = dict(iter_count=iters, converged=fired, history=history, elapsed=elapsed, residual_norm=[], rhs_norm=[],
                   solution=None)
        for j in range(nreal):
            res_sq = sum(comm.allgather_scalars({me: parts[me][j] for me, _ in locals_}))
            rhs_sq = sum(comm.allgather_scalars({me: float(np.sum(interior[me][:, j] ** 2)) for me, _ in locals_}))
            out["residual_norm"].append(float(np.sqrt(res_sq)))
            out["rhs_norm"].append(float(np.sqrt(rhs_sq)))
        if gather_solution:
            pieces = {me: np.ascontiguousarray(sd.batch_get_interior(stream)[:, :nreal]) for me, sd in locals_}
            out["solution"] = comm.gather_vectors(pieces)
        return out

    def solve_many(self, rhs, gather_solution=True):
        """Several right-hand sides against the matrix initialize() set up, solved in blocks of up to eight columns that
        share every pass over the local matrices and every launch of the outer step (an extension: the reference
        solves one system).  `rhs`: a host array of shape (global_size, nrhs), the same on every rank, indexed by the
        caller's row ids like initialize(rhs=...).  The columns run in blocks of 8, the last block padded to 2, 4 or 8
        with zero columns whose results are dropped.  Per block a synchronous loop of its own: exchange, boundary
        update, per-column check, local solve, restriction -- no speculative solve, no early exchange.  A column whose
        convergence test fires is frozen from then on, in the local solves and in the restriction: its solution is the
        iterate at which a run on that column alone would have stopped.  The single-right-hand-side state is untouched.
        Returns per-column lists iter_count, converged, residual_norm, rhs_norm and history (the global residual sum
        per iteration), solution of shape (global_size, nrhs) on the root rank, and elapsed (the loops of the blocks).
        Collective like run(): every rank calls it."""
        B = self._check_batch(rhs)
        nrhs = B.shape[1]
        out = dict(iter_count=[], converged=[], residual_norm=[], rhs_norm=[], history=[], elapsed=0.0, solution=None)
        sols, at = [], 0
        for k in batch_blocks(nrhs):
            part = self._solve_block(B[:, at:at + min(k, nrhs - at)], k, gather_solution)
            at += k
            for key in ("iter_count", "converged", "residual_norm", "rhs_norm", "history"):
                out[key] += part[key]
            out["elapsed"] += part["elapsed"]
            sols.append(part["solution"])
        if gather_solution and all(p is not None for p in sols):
            out["solution"] = np.concatenate(sols, axis=1)
        return out

    def run(self, gather_solution=True):
        """SchwarzBase::run (schwarz_base.cpp:323-506).  Returns a dict with the
        solution (on the root rank) and the run statistics."""
        m, be, comm = self.metadata, self.backend, self.comm
        if outer.wants_fgmres(self.settings, m, comm):
            return outer.run_fgmres(self, gather_solution)
        self.begin_run()
        be.synchronize()
        comm.barrier()
        start = time.perf_counter()
        while m.iter_count < m.max_iters:
            if self.step():
                break
        be.synchronize()
        comm.barrier()  # schwarz_base.cpp:453
        elapsed = time.perf_counter() - start
        return self.finish_run(elapsed, gather_solution)
