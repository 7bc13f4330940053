"""schwz_amd -- MI355X-native Restricted Additive Schwarz hot path.

Host-side mirror of the schwarz-lib solver API (Settings / Metadata / SolverRAS)
over libschwz_hip.so (include/schwz_hip.h).  Importing the package loads the
shared library and fails loudly if it has not been built.
"""
from . import _capi as capi  # noqa: F401  (loads libschwz_hip.so)
from ._capi import SchwzError, NotImplementedSchwz  # noqa: F401
from .comm import InProcessComm, TorchDistComm, WindowComm  # noqa: F401
from .core import Coarse, Outer, dense_inverse, outer_copy  # noqa: F401
from .core import (BatchCg, Bicgstab, Chebyshev, Csr, DeviceWindow, Gmres, Pcg, PcgF32, PeerWindow, Problem, Subdomain, Trs, TrsLU, TrsSweeps, cholesky, gather, ilu0, isai, lu, parilu,  # noqa: F401
                   scatter,
                   partition_regular, partition_regular2d, rhs_random)
from .solver import (HipBackend, Metadata, Settings, SolverRAS, batch_blocks,  # noqa: F401
                     PARTITION_CUSTOM, PARTITION_METIS, PARTITION_REGULAR, PARTITION_REGULAR2D,
                     SOLVER_DIRECT_CHOLMOD, SOLVER_DIRECT_GINKGO, SOLVER_DIRECT_UMFPACK,
                     SOLVER_ITERATIVE_GINKGO)

__all__ = ["Settings", "Metadata", "SolverRAS", "HipBackend", "InProcessComm", "TorchDistComm", "WindowComm",
           "Problem", "Subdomain", "Csr", "Pcg", "Trs", "SchwzError"]
