"""The cases tests/test_joint_twin.py (on the CPU, with the twin) and tests/test_gpu_joint.py (on the device) share: the
rows of the optimizer comparison and the hand-derived case of tests/golden/JOINT_ANALYTIC.md."""
import numpy as np

from grad_traj_optimization_amd import problem

SCENE = dict(grid=(60, 50, 30), density=0.03, seed=11)      # the scene of tests/test_gpu_time.py
# the optimizer against the serial restatement: B rows of m segments, 12 evaluations.  The seeds are chosen so that
# tests/test_joint_twin.py::test_optimizer_cases_have_no_near_ties holds (no accept / reject decision of the twin's run
# within 1e-6 of a tie)
SERIAL_B, SERIAL_EVALS = 4, 12
SERIAL_SEEDS = {3: 7103, 6: 7206}
SERIAL_OPT = dict(rho=2.0, t_min=0.1, t_max=4.0, max_evals=SERIAL_EVALS)
TIE = 1e-6


def scene_map():
    return problem.make_map(SCENE["grid"], density=SCENE["density"], seed=SCENE["seed"])


def serial_case(m, mp):
    """(batch, lb, ub, T_lo) of the comparison on m segments: collision rows, default bounds, one pinned segment."""
    from grad_traj_optimization_amd import GtopContext
    b = problem.make_trajectories(SERIAL_B, m, mp, seed=SERIAL_SEEDS[m], step_len=(1.0, 2.0), boundary="random")
    lb, ub = GtopContext.default_bounds(b.waypoints)
    T_lo = np.zeros((SERIAL_B, m))
    T_lo[:, 1] = SERIAL_OPT["t_max"] + 0.5          # segment 1 pinned above t_max
    return b, lb, ub, T_lo


# ---- tests/golden/JOINT_ANALYTIC.md ----
ANALYTIC = dict(L=3.0, ws=1.0, rho=2.0)
ANALYTIC_EVALS = 30
ANALYTIC_START_T = (1.5, 3.5)
ANALYTIC_OPT = dict(rho=ANALYTIC["rho"], t_min=0.1, t_max=10.0, max_evals=ANALYTIC_EVALS)
# the twin's run ends (F - F*) / F* = ANALYTIC_TWIN_GAP above the optimum (measured: JOINT_ANALYTIC.md); the device is
# held to ANALYTIC_MARGIN times that
ANALYTIC_TWIN_GAP = 7.450860257339419e-05
ANALYTIC_MARGIN = 2.0


def analytic_answer():
    L, ws, rho = ANALYTIC["L"], ANALYTIC["ws"], ANALYTIC["rho"]
    tau = (3600.0 * ws * L * L / rho) ** (1.0 / 6.0)
    return dict(tau=tau, T=np.array([tau / 2, tau / 2]), v=15.0 * L / (8.0 * tau), a=0.0,
                F=720.0 * ws * L * L / tau ** 5 + rho * tau)


def analytic_case():
    """(Df (3, 6), x0 (9,), lb, ub): rest to rest along x over L, the junction's position pinned at L / 2 by lb = ub,
    its velocity and acceleration free in +-10."""
    L = ANALYTIC["L"]
    Df = np.zeros((3, 6))
    Df[0, 3] = L
    x0 = np.zeros((3, 3))
    x0[0, 0] = L / 2
    lb, ub = np.full((3, 3), -10.0), np.full((3, 3), 10.0)
    lb[:, 0] = ub[:, 0] = x0[:, 0]
    return Df, x0.reshape(-1), lb.reshape(-1), ub.reshape(-1)
