// schwz::Settings / schwz::Metadata -- the structs the driver fills from its flags
// (benchmarking/bench_ras.cpp:50-150).  Field names, types and defaults follow the reference's
// include/settings.hpp:77-496 so that driver code written against it compiles unchanged; members
// that only made sense for the replicated-global-matrix design (N-long index maps) are absent.
#pragma once

#include <mpi.h>

#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include <ginkgo/ginkgo.hpp>

#define MINIMAL_OVERLAP 2

namespace schwz {

struct Settings {
    std::string executor_string;
    std::shared_ptr<gko::Executor> executor = gko::ReferenceExecutor::create();

    enum partition_settings {
        partition_regular = 0x0,
        partition_regular2d = 0x4,
        partition_metis = 0x1,
        partition_zoltan = 0x2,
        partition_custom = 0x3
    };
    partition_settings partition = partition_settings::partition_regular;

    gko::int32 overlap = MINIMAL_OVERLAP;
    std::string matrix_filename = "null";
    bool explicit_laplacian = true;
    bool use_mixed_precision = false;
    bool enable_random_rhs = false;
    bool print_matrices = false;
    bool debug_print = false;

    enum local_solver_settings {
        direct_solver_cholmod = 0x0,
        direct_solver_umfpack = 0x5,
        direct_solver_ginkgo = 0x1,
        iterative_solver_ginkgo = 0x2,
        iterative_solver_dealii = 0x3,
        solver_custom = 0x4
    };
    local_solver_settings local_solver = local_solver_settings::iterative_solver_ginkgo;

    bool non_symmetric_matrix = false;
    unsigned int restart_iter = 1u;
    int reset_local_crit_iter = -1;
    bool naturally_ordered_factor = false;
    std::string metis_objtype;
    bool use_precond = false;
    bool write_debug_out = false;
    bool write_iters_and_residuals = false;
    bool enable_logging = false;
    bool write_perm_data = false;
    int shifted_iter = 1;

    struct comm_settings {
        bool enable_onesided = false;
        bool enable_overlap = false;
        bool enable_put = false;
        bool enable_get = true;
        bool stage_through_host = false;
        bool enable_one_by_one = false;
        bool enable_flush_local = false;
        bool enable_flush_all = true;
        bool enable_lock_local = false;
        bool enable_lock_all = true;
    };
    comm_settings comm_settings;

    struct convergence_settings {
        bool put_all_local_residual_norms = true;
        bool enable_global_simple_tree = false;
        bool enable_decentralized_leader_election = false;
        bool enable_global_check = true;
        bool enable_accumulate = false;
        bool enable_global_check_iter_offset = false;
        enum local_convergence_crit { residual_based = 0x0, solution_based = 0x1 };
        local_convergence_crit convergence_crit = local_convergence_crit::solution_based;
    };
    convergence_settings convergence_settings;

    std::string factorization = "cholmod";
    std::string reorder;

    Settings(std::string executor_string = "reference") : executor_string(std::move(executor_string)) {}
};


template <typename ValueType, typename IndexType>
struct Metadata {
    MPI_Comm mpi_communicator;
    gko::size_type global_size = 0;
    gko::size_type oned_laplacian_size = 0;
    gko::size_type local_size = 0;
    gko::size_type local_size_x = 0;
    gko::size_type local_size_o = 0;
    gko::size_type overlap_size = 0;
    gko::size_type num_subdomains = 1;
    int my_rank = 0;
    int my_local_rank = 0;
    int local_num_procs = 1;
    int comm_size = 1;
    int num_threads = 1;
    IndexType iter_count = 0;
    ValueType tolerance = 0;
    ValueType local_solver_tolerance = 0;
    IndexType max_iters = 0;
    IndexType local_max_iters = -1;
    IndexType updated_max_iters = -1;
    std::string local_precond = "null";
    unsigned int precond_max_block_size = 16;
    // extensions: ParILU options of the ilu / isai local preconditioner (schwz_solver_options): factors from
    // par_ilu_sweeps ParILU sweeps on the GPU (ilu, isai), factors applied by trisolve_sweeps Jacobi sweeps
    // (ilu); 0 = the exact ILU(0) and exact triangular solves
    int par_ilu_sweeps = 0;
    int trisolve_sweeps = 0;
    // extension: "single" runs the iterative local solve as fp32 CG on the fp64 start residual, the correction
    // added in fp64 (schwz_ras_set_local_precision); CG without a preconditioner or with scalar Jacobi only
    std::string local_solver_precision = "double";
    // extension: the Krylov method of the iterative local solve of a non-symmetric matrix: "gmres"
    // (GMRES(restart_iter), the reference's) or "bicgstab" (schwz_ras_set_nonsym_solver); without
    // non_symmetric_matrix or with a direct local solver it has no effect, like restart_iter
    std::string non_symmetric_solver = "gmres";
    // extension: the type GMRES stores its Krylov basis in: "double", or "single" for compressed-basis GMRES
    // (schwz_ras_set_gmres_basis: fp32 basis vectors, fp64 arithmetic, blocked CGS2; inside one cycle the true
    // residual follows the recurred norm the stop test sees only to about 2^-24 of the cycle's start residual).
    // Without non_symmetric_matrix, with a direct local solver or with non_symmetric_solver "bicgstab" it has no
    // effect, like restart_iter
    std::string gmres_basis = "double";
    // extension: the method of the iterative local solve of a symmetric matrix: "cg" (the reference's) or "chebyshev"
    // (schwz_ras_set_sym_solver: local_precond null or block-jacobi of block size 1, double precision); with
    // non_symmetric_matrix or a direct local solver it has no effect, like restart_iter.  Bounds on the spectrum of
    // M^-1 A: 0 means automatic (lambda_max: the Gershgorin bound of the local matrix, lambda_min: lambda_max /
    // chebyshev_eig_ratio), explicit values override either end.  Beyond the defaults the bounds are the user's
    // responsibility: a lambda_max below the true one makes the local iteration diverge.
    std::string symmetric_solver = "cg";
    double chebyshev_eig_ratio = 30.0;
    double chebyshev_lambda_min = 0.0;
    double chebyshev_lambda_max = 0.0;
    // extensions (the reference has one level only): the coarse space of a two-level RAS.  "none", or "aggregates":
    // at the start of every outer step, after the halo exchange, x <- x + Z A0^-1 Z^T (b - A x), A0 = Z^T A Z, Z the
    // 0/1 matrix of a partition of the rows into at most 4096 aggregates, each inside one subdomain's interior.
    // coarse_aggregate_vector: one id >= 0 per global row in the caller's row ids (rows of one id in different
    // subdomains become different aggregates); empty: coarse_aggregates > 0 parts of every subdomain's interior
    // graph.  Synchronous two-sided loop only, overlap >= 2 on more than one subdomain.
    std::string coarse_space = "none";
    int coarse_aggregates = 0;
    std::vector<long long> coarse_aggregate_vector;
    ValueType current_residual_norm = -1.0;
    ValueType min_residual_norm = -1.0;

    // (id, rank, count, name, samples): filled by MEASURE_ELAPSED_FUNC_TIME in the reference
    std::vector<std::tuple<int, int, int, std::string, std::vector<ValueType>>> time_struct;
    // per subdomain: (rank, [(from, n)], [(to, n)], num_in, num_out)
    std::vector<std::tuple<int, std::vector<std::tuple<int, int>>, std::vector<std::tuple<int, int>>, int, int>>
        comm_data_struct;

    struct post_process_data {
        std::vector<std::vector<ValueType>> global_residual_vector_out;
        std::vector<ValueType> local_residual_vector_out;
        std::vector<ValueType> local_converged_iter_count;
        std::vector<ValueType> local_converged_resnorm;
        std::vector<ValueType> local_timestamp;
    };
    post_process_data post_process_data;
    double init_mpi_wtime = 0.0;

    // contiguous ownership ranges, length num_subdomains+1 (the reference's first_row array)
    std::vector<long long> first_row;
    // new->old permutation when a partition vector was applied (empty otherwise)
    std::vector<long long> permutation;
};

}  // namespace schwz
