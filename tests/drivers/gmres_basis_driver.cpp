// Test driver for the basis type of the local GMRES of the C++ mirror (Metadata::gmres_basis, an extension of the
// reference's Metadata): a RAS run on a Matrix-Market file with non_symmetric_matrix set, the local systems solved by
// GMRES(restart_iter) with scalar Jacobi, the Krylov basis stored in fp64 ("double") or in fp32 ("single").  Usage
// under mpiexec:
//   gmres_basis_driver <double|single|any other name> <matrix file> <tol> <max_iters> <restart_iter> [gmres|bicgstab]
// Prints what SolverRAS::run prints (numbers with 17 digits: the " residual norm" line is what the test compares)
// plus one line "RESULT iters=<k> solnorm=<|x|_2>" on rank 0; a refused name prints "REFUSED <what>" and exits
// with status 3.
#include <mpi.h>

#include <cmath>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>

#include <restricted_schwarz.hpp>

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::cerr << "usage: gmres_basis_driver double|single matrix_file tol max_iters restart_iter [gmres|bicgstab]"
                  << std::endl;
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
        metadata.gmres_basis = argv[1];
        if (argc > 6) metadata.non_symmetric_solver = argv[6];
        metadata.local_precond = "block-jacobi";
        metadata.precond_max_block_size = 1;
        metadata.tolerance = std::atof(argv[3]);
        metadata.max_iters = std::atoi(argv[4]);
        metadata.local_solver_tolerance = 1e-12;
        metadata.local_max_iters = -1;
        settings.matrix_filename = argv[2];
        settings.explicit_laplacian = false;
        settings.non_symmetric_matrix = true;
        settings.restart_iter = std::atoi(argv[5]);
        settings.overlap = 2;
        settings.convergence_settings.enable_global_check = true;
        settings.local_solver = schwz::Settings::local_solver_settings::iterative_solver_ginkgo;
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
            double sq = 0.0;
            for (gko::size_type i = 0; i < solution->get_size()[0]; ++i) sq += solution->at(i) * solution->at(i);
            std::cout << "RESULT iters=" << metadata.iter_count << " solnorm=" << std::sqrt(sq) << std::endl;
        }
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << std::endl;
        rc = 1;
    }
    MPI_Finalize();
    return rc;
}
