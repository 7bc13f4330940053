// Test driver for the choice of the symmetric local solver of the C++ mirror (Metadata::symmetric_solver, an
// extension of the reference's Metadata): a 2-D Laplacian RAS run whose local systems are solved by CG or by the
// Chebyshev iteration with its default bounds, scalar Jacobi, a fixed number of inner iterations.  Usage under mpiexec:
//   cheb_driver <cg|chebyshev|any other name> <grid edge n> <tol> <max_iters> <local_max_iters>
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
        std::cerr << "usage: cheb_driver cg|chebyshev n tol max_iters local_max_iters" << std::endl;
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
        metadata.symmetric_solver = argv[1];
        metadata.local_precond = "block-jacobi";
        metadata.precond_max_block_size = 1;
        metadata.oned_laplacian_size = std::atoi(argv[2]);
        metadata.tolerance = std::atof(argv[3]);
        metadata.max_iters = std::atoi(argv[4]);
        metadata.local_solver_tolerance = 0.0;
        metadata.local_max_iters = std::atoi(argv[5]);
        settings.explicit_laplacian = true;
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
