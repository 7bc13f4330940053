// Test driver for the two-level RAS of the C++ mirror (Metadata::coarse_space / coarse_aggregates /
// coarse_aggregate_vector, extensions of the reference's Metadata): the n x n x n Laplacian in z-slabs, one per rank,
// direct local solves, with the aggregation coarse correction on boxes of bx x by x bz cells (numbered z-layer of
// boxes after z-layer) or without it.  Usage under mpiexec:
//   coarse_driver <none|aggregates|any other name> <n> <bx> <by> <bz> <tol> <max_iters> [auto <aggregates per rank>]
// Prints what SolverRAS::run prints plus, on rank 0, "RESULT iters=<k>" and "HIST <G_0> <G_1> ..." (the sums of the
// ranks' local residual norms per outer iteration, 17 digits); a refused name prints "REFUSED <what>", exit status 3.
#include <mpi.h>

#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>

#include <restricted_schwarz.hpp>

int main(int argc, char **argv)
{
    if (argc < 8) {
        std::cerr << "usage: coarse_driver none|aggregates n bx by bz tol max_iters [auto k]" << std::endl;
        return 2;
    }
    MPI_Init(&argc, &argv);
    int rc = 0;
    try {
        schwz::Settings settings("hip");
        schwz::Metadata<double, int> metadata;
        metadata.mpi_communicator = MPI_COMM_WORLD;
        MPI_Comm_rank(MPI_COMM_WORLD, &metadata.my_rank);
        MPI_Comm_size(MPI_COMM_WORLD, &metadata.comm_size);
        metadata.num_subdomains = metadata.comm_size;
        const int n = std::atoi(argv[2]), bx = std::atoi(argv[3]), by = std::atoi(argv[4]), bz = std::atoi(argv[5]);
        metadata.coarse_space = argv[1];
        if (argc >= 10 && std::string(argv[8]) == "auto") {
            metadata.coarse_aggregates = std::atoi(argv[9]);
        } else if (metadata.coarse_space != "none") {
            const int cx = (n + bx - 1) / bx, cy = (n + by - 1) / by;
            for (int z = 0; z < n; ++z)
                for (int y = 0; y < n; ++y)
                    for (int x = 0; x < n; ++x) metadata.coarse_aggregate_vector.push_back(((z / bz) * cy + y / by) * cx + x / bx);
        }
        metadata.tolerance = std::atof(argv[6]);
        metadata.max_iters = std::atoi(argv[7]);
        settings.matrix_filename = "poisson3d:" + std::to_string(n);
        settings.explicit_laplacian = false;
        settings.overlap = 2;
        settings.convergence_settings.enable_global_check = true;
        settings.local_solver = schwz::Settings::local_solver_settings::direct_solver_ginkgo;
        schwz::SolverRAS<double, int> solver(settings, metadata);
        try {
            solver.initialize();
        } catch (const BadDimension &e) {
            if (metadata.my_rank == 0) std::cout << "REFUSED " << e.what() << std::endl;
            MPI_Finalize();
            return 3;
        }
        std::shared_ptr<gko::matrix::Dense<double>> solution;
        std::cout.precision(17);
        solver.run(solution);
        if (metadata.my_rank == 0) {
            std::cout << "RESULT iters=" << metadata.iter_count << std::endl;
            const auto &h = metadata.post_process_data.global_residual_vector_out;
            std::cout << "HIST";
            for (size_t k = 0; !h.empty() && k < h[0].size(); ++k) {
                double g = 0.0;
                for (size_t p = 0; p < h.size(); ++p) g += h[p][k];
                std::cout << " " << g;
            }
            std::cout << std::endl;
        }
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << std::endl;
        rc = 1;
    }
    MPI_Finalize();
    return rc;
}
