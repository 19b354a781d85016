"""Drop-in module (reference NewtonSolver.py): Newton solvers run by libipm355.so."""
from ipm355.newton import (NewtonSolver, NewtonSolverCG, NewtonSolverCholesky, NewtonSolverCholeskyDual,  # noqa: F401
                           NewtonSolverCholeskyDualQP, NewtonSolverCholeskyDualQPInfeasibleStart, NewtonSolverDiagonal,
                           NewtonSolverDirect, NewtonSolverNPLstSq, NewtonSolverNPSolve)
