"""quflow_amd -- MI355X-native implementation of quflow's isospectral hot path.

Drop-in for the reference's stepper and Laplacian-backend protocols
(SURVEY.md section 8b):

    import quflow_amd as qfa
    W = qfa.isomp(W, dt, steps=100, stats=stats)        # quflow.integrators.isomp
    P = qfa.solve_poisson(W); W2 = qfa.laplace(P)       # quflow.laplacian
    qfa.laplacian  -> module with solve_poisson / laplace / laplacian / select_skewherm
    qfa.IsompHIP(N, dtype), qfa.PoissonHIP(N, dtype)    # device-object form (runfile selection)

All compute runs in hand-written HIP kernels for gfx950 behind the C ABI of
include/quflow_hip.h; there is no CPU fallback.
"""

from . import laplacian
from . import integrators
from . import physics
from . import geometry
from . import ensemble
from . import quantization
from . import transforms
from . import sht
from . import analysis
from . import linalg
from . import dynamics
from . import simulation
from .simulation import Simulation, solve, create_runfile
QuSimulation = Simulation          # the reference's name (quflow/simulation.py:60): scripts that say qf.QuSimulation run unchanged
from .quantization import (shr2mat, mat2shr, shc2mat, mat2shc, get_basis, compute_basis, basis_break_index, elm2ind, ind2elm,
                           berezin_multipliers, elmr2mat, elmc2mat)
from .transforms import (shr2fun, shc2fun, shr2shc, shc2shr, as_fun, as_shr, sphgrid, fun2img, img2fun, fun2shr,
                         fun2shc, state_fields)
from .geometry import hbar, bracket, norm_L2, inner_L2, norm_Linf, norm_L1, integral, qtime2seconds, seconds2qtime
from .geometry import so3_generators, cartesian_generators, rotate, rotation_matrix, grad
from .dynamics import blob, north_blob, project_el
from .laplacian import (solve_poisson, laplace, PoissonHIP, solve_heat, solve_helmholtz, solve_viscdamp,
                        solve_globalqg, ViscDampStep, TridiagonalHamiltonian, coriolis, AffineForcing, StochasticForcing)
from .integrators import (isomp, isomp_fixedpoint, IsompHIP, DeviceTrajectory, DeviceEnsemble, DeviceStackTrajectory,
                          DeviceMHDTrajectory, euler, heun, rk4,
                          isomp_simple, isomp_quasinewton, magmp, magmp_fixedpoint, solve_mhd,
                          commutator, commutator_generic, commutator_skewherm, estimate_stepsize, project_skewherm)
from .analysis import scale_decomposition
from .physics import (energy_euler, casimirs, mhd_diagnostics, energy_mhd, cross_helicity, magnetic_energy, enstrophy, inner_Hm1, norm_Hm1, inner_H1, norm_H1, sectional_curvature)
from .context import get_context, set_device, release_contexts, guard_report
from ._lib import QuflowHipError, device_count, device_info

__version__ = "0.1.0"
