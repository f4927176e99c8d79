"""AdvectionDiffusionImplicit::euler (main.cpp:10030-10118) restated in plain NumPy, from the reference's text alone: the five pointwise
passes around KernelAdvect, KernelDiffusionRHS and the three DiffusionSolver::solve calls.

  euler(vel, pres, h, dt, nu, advect, diffusion_rhs, solver)

advect (compute<VectorLab>(KernelAdvect), 10038: vel -> (vel', tmpV)), diffusion_rhs (KernelDiffusionRHS, 10058: vel -> tmpV) and solver
(mmysolver.solve(), 10096: (rhs, x0, direction) -> x) are callables the caller passes in; arrays are [nb, 8, 8, 8(, 3)], h is the spacing per
block.  Every pass is written in the reference's association and evaluated in float64, one rounding per operation:

  10053-10055   V    = TMPV * ih3 + V                                   ih3 = 1.0 / (h * h * h)
  10068-10076   TMPV = -TMPV * ih3 + (V - velocity) / (dt * nu)
  10092-10093   P = 0 ;  RHS = h3 * TMPV.u[index]                       h3 = h * h * h
  10104         V.u[index] += P
  10115         P = pressure                                            (saved at 10049)

so with bit-exact callables every returned array is the reference's bit for bit.  Returned: dict(vel, tmpV, rhs = the three right-hand
sides, pres = the restored pressure, guess = V after 10055, solutions = the three P).

`mutation` selects one deliberately wrong step of MUTATIONS (tests/test_helmholtz_restatement.py shows which arrays each one moves, and
that the solver-tolerance comparison of tests/test_gpu_amr.py cannot see pres_not_zeroed and guess_left_out)."""
import numpy as np

f64 = np.float64
MUTATIONS = ("pres_not_zeroed", "direction_0_face_rule", "guess_left_out", "ih3_of_the_neighbour", "added_to_the_next_component",
             "pres_not_restored", "reciprocal_of_dt_nu")


def euler(vel, pres, h, dt, nu, advect, diffusion_rhs, solver, mutation=None):
    assert mutation is None or mutation in MUTATIONS, mutation
    h = np.asarray(h, dtype=np.float64)
    per_block = lambda a: a.reshape(-1, 1, 1, 1)
    h3 = h * h * h                                                        # 10085
    hh = np.roll(h, 1) if mutation == "ih3_of_the_neighbour" else h      # the spacing of the block one slot before
    ih3 = f64(1.0) / (hh * hh * hh)                                       # 10044, 10063
    ih3v = per_block(ih3)[..., None]
    pressure = np.array(pres, dtype=np.float64)                           # 10049
    V, TMPV = advect(np.array(vel, dtype=np.float64))                     # 10038
    velocity = V.copy()                                                   # 10050-10052
    if mutation != "guess_left_out":
        V = TMPV * ih3v + V                                               # 10053-10055
    guess = V.copy()
    TMPV = diffusion_rhs(V)                                               # 10058
    dtnu = f64(dt) * f64(nu)
    if mutation == "reciprocal_of_dt_nu":
        TMPV = -TMPV * ih3v + (V - velocity) * (f64(1.0) / dtnu)
    else:
        TMPV = -TMPV * ih3v + (V - velocity) / dtnu                       # 10068-10076
    P = pressure.copy()
    rhs, solutions = [], []
    V = V.copy()
    for index in range(3):                                                # 10080
        if mutation != "pres_not_zeroed":
            P = np.zeros_like(pressure)                                   # 10092
        RHS = per_block(h3) * TMPV[..., index]                            # 10093
        rhs.append(RHS)
        P = solver(RHS, P, 0 if mutation == "direction_0_face_rule" else index)   # 10081, 10096
        solutions.append(P)
        to = (index + 1) % 3 if mutation == "added_to_the_next_component" else index
        V[..., to] = V[..., to] + P                                       # 10104
    if mutation != "pres_not_restored":
        P = pressure.copy()                                               # 10115
    return dict(vel=V, tmpV=TMPV, rhs=rhs, pres=P, guess=guess, solutions=solutions)
