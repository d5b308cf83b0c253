"""MI355X-native hot path of the path-space PDE solver.

The directory can be used in two ways:
  * as a package:      ``from path_space_pde_solver_amd import Solver, LLGC``
    (``path_space_pde_solver_amd/`` at the repo root is a thin import shim because this
    directory's name is not a valid Python identifier);
  * flat, like the reference: put this directory on ``sys.path`` and
    ``from solver import Solver``; ``from problems import LLGC`` -- the module names the
    reference's notebooks import.
"""
from .function_space import (Affine, Constant, DenseNet, DenseNet_tanh, DenseNet_tanh_2, Linear, MySequential,  # noqa: F401
                             SingleParam)
from .problems import (LLGC, LQGC, AllenCahn, DoubleWell, DoubleWell_multidim,  # noqa: F401
                       DoubleWell_OU, DoubleWell_multidim_2, DoubleWell_multidim_3, LLGC_general_f,
                       DoubleWell_multidim_for_general_solver, HeatEquation, ExponentialOnSphere,
                       ExponentialOnBallNonlinear, ExponentialOnBallNonlinearSin,
                       ExponentialOnBallNonlinearSinHessian,
                       ExponentialOnSphereNonlinearParabolic, QuadraticOnBox, Committor,
                       ExponentialOnSphereParabolic, DoubleWell_stopping, DoubleWell_stopping_linear,
                       DoubleWell_expectation_hitting_time, Committor_DoubleWell, QuadraticGradient, Helmholtz, Oscillations,
                       SinNorm2, FokkerPlanckEigenvalue, SchroedingerEigenvalue)
from .solver import Solver  # noqa: F401
from .general_solver import GeneralSolver, EllipticSolver  # noqa: F401
from .eigenvalue_solver import EigenvalueSolver  # noqa: F401
from .plan_native import PlanUnsupported  # noqa: F401
from . import native  # noqa: F401
from . import native_shapes  # noqa: F401
from . import plan_native, plan_dense_native, plan_general_native, plan_value_native, plan_pinn_native  # noqa: F401
from .utilities import do_importance_sampling_me, loss_relative_errors  # noqa: F401

__all__ = ['Solver', 'GeneralSolver', 'EllipticSolver', 'ExponentialOnSphere', 'ExponentialOnBallNonlinear',
           'ExponentialOnBallNonlinearSin', 'ExponentialOnBallNonlinearSinHessian', 'ExponentialOnSphereNonlinearParabolic', 'QuadraticOnBox', 'Committor', 'LLGC', 'LQGC', 'DoubleWell', 'DoubleWell_multidim', 'DoubleWell_OU', 'DoubleWell_multidim_2', 'DoubleWell_multidim_3', 'LLGC_general_f', 'DoubleWell_multidim_for_general_solver',
           'AllenCahn', 'HeatEquation', 'MySequential', 'DenseNet', 'DenseNet_tanh', 'DenseNet_tanh_2', 'SingleParam',
           'Constant', 'Linear', 'Affine', 'PlanUnsupported', 'native', 'ExponentialOnSphereParabolic', 'DoubleWell_stopping',
           'DoubleWell_stopping_linear', 'DoubleWell_expectation_hitting_time', 'Committor_DoubleWell', 'QuadraticGradient',
           'Helmholtz', 'Oscillations', 'SinNorm2', 'FokkerPlanckEigenvalue', 'SchroedingerEigenvalue', 'EigenvalueSolver']
