// Test driver for the mixed-precision local solve of the C++ mirror (Metadata::local_solver_precision, an
// extension of the reference's Metadata): a 2-D Laplacian RAS run whose local CG runs in fp64 or as fp32 CG on
// the fp64 start residual.  Usage under mpiexec:
//   mixed_driver <double|single> <precond> <grid edge n> <tol> <max_iters>
// <precond>: null, block-jacobi (block size 1), block-jacobi:<block size>, ilu, isai.
// Prints what SolverRAS::run prints plus one line "RESULT iters=<k> solnorm=<|x|_2>" on rank 0; a refused
// combination prints "REFUSED <what>" and exits with status 3.
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
        std::cerr << "usage: mixed_driver double|single precond n tol max_iters" << std::endl;
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
        metadata.local_solver_precision = argv[1];
        std::string precond = argv[2];
        metadata.precond_max_block_size = 1;
        const size_t colon = precond.find(':');
        if (colon != std::string::npos) {
            metadata.precond_max_block_size = (unsigned)std::atoi(precond.c_str() + colon + 1);
            precond = precond.substr(0, colon);
        }
        metadata.local_precond = precond;
        metadata.oned_laplacian_size = std::atoi(argv[3]);
        metadata.tolerance = std::atof(argv[4]);
        metadata.max_iters = std::atoi(argv[5]);
        metadata.local_solver_tolerance = 1e-10;
        metadata.local_max_iters = -1;
        settings.explicit_laplacian = true;
        settings.convergence_settings.enable_global_check = true;
        settings.local_solver = schwz::Settings::local_solver_settings::iterative_solver_ginkgo;
        schwz::SolverRAS<double, int> solver(settings, metadata);
        try {
            solver.initialize();
        } catch (const NotImplemented &e) {
            if (metadata.my_rank == 0) std::cout << "REFUSED " << e.what() << std::endl;
            MPI_Finalize();
            return 3;
        }
        std::shared_ptr<gko::matrix::Dense<double>> solution;
        solver.run(solution);
        if (metadata.my_rank == 0) {
            double sq = 0.0;
            for (gko::size_type i = 0; i < solution->get_size()[0]; ++i) sq += solution->at(i) * solution->at(i);
            std::cout.precision(17);
            std::cout << "RESULT iters=" << metadata.iter_count << " solnorm=" << std::sqrt(sq) << std::endl;
        }
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << std::endl;
        rc = 1;
    }
    MPI_Finalize();
    return rc;
}
