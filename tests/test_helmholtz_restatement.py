"""The two NumPy statements the implicit-diffusion path of the device is held to -- pinned WITHOUT a device before anything is judged by them:

  * tests/bicgstab_restatement.py run as DiffusionSolver::solve (main.cpp:6896-7146: the same routine as PoissonSolverAMR::solve on the
    Helmholtz operator of one velocity component, no mean constraint, no cap on the breakdown restarts) with the oracle's diff_lhs /
    diff_precond IS the oracle's diff_solve (itself pinned to the compiled reference by tests/test_oracle_amr.py): every bit of the
    solution, the iteration count and the restart count -- across a restart (directions 0 and 2 of `l012`) and across the k = 50 refresh
    (direction 1);
  * tests/implicit_step_restatement.py with the oracle's advect_implicit, diffusion_rhs and either solver IS the oracle's
    advdiff_implicit, in both of its advect modes;
  * what the device sweeps of tests/test_gpu_helmholtz_iteration.py need of their inputs holds on the oracle;
  * each deliberately wrong step of implicit_step_restatement.MUTATIONS changes a returned array on every input the device tests use --
    or is listed as not applicable with the reason -- and two of them stay below the 1e-6 x change bound of
    tests/test_gpu_amr.py::test_implicit_diffusion_solver: that test cannot see them, a bitwise comparison cannot miss them."""
import numpy as np
import pytest

import bicgstab_restatement as R
import helmholtz_cases as H
import implicit_step_restatement as S

TIGHT = (1e-12, 1e-11)


def _restated_solve(c, direction, rhs=None, x0=None, max_restarts=H.UNBOUNDED, tol=TIGHT[0], tol_rel=TIGHT[1]):
    return R.solve(c.rhs if rhs is None else rhs, c.x0 if x0 is None else x0, c.A(direction), c.Minv, "sequential", None, tol, tol_rel,
                   max_restarts=max_restarts)


def _first_restart(c, direction, M):
    """(norms of iterations 1 .. M, the loop pass k in which the first restart happens or None) at tol = tol_rel = 0"""
    A, Minv = c.A(direction), c.Minv
    st = R.init(c.rhs, c.x0, A, Minv)
    norms, first = [], None
    for k in range(M):
        st = R.iteration(st, k, A, Minv, max_restarts=H.UNBOUNDED)
        norms.append(float(st["norm"]))
        if st["restarted"] and first is None:
            first = k
    return norms, first


def _rises(norms):
    return any(b >= a for a, b in zip(norms, norms[1:]))


# ------------------------------------------------------------------ check 1: the solver

@pytest.mark.parametrize("direction", [0, 1, 2])
def test_solver_is_the_oracles_bit_for_bit_on_the_three_level_mesh(direction):
    """`l012`: 40 / 66 / 40 iterations; directions 0 and 2 restart (once, in loop pass k = 31), direction 1 nowhere and passes k = 50"""
    c = H.case("l012")
    p, its, restarts = c.oracle_solve(direction, *TIGHT)
    x, k, st = _restated_solve(c, direction)
    print(f"l012, direction {direction}: oracle {its} iterations / {restarts} restarts, restatement {k} / {st['restarts']}")
    assert (k, st["restarts"]) == (its, restarts)
    assert np.array_equal(x, p), np.abs(x - p).max()
    assert its == (40, 66, 40)[direction]
    assert (restarts >= 1) == (direction != 1)


@pytest.mark.parametrize("direction", [0, 1, 2])
def test_solver_is_the_oracles_bit_for_bit_on_the_mixed_uniform_grid(direction):
    c = H.case("mixed16", direction)
    p, its, restarts = c.oracle_solve(direction, *TIGHT)
    x, k, st = _restated_solve(c, direction)
    print(f"mixed16, direction {direction}: oracle {its} iterations / {restarts} restarts, restatement {k} / {st['restarts']}")
    assert (k, st["restarts"]) == (its, restarts) and its > 8
    assert np.array_equal(x, p), np.abs(x - p).max()


def test_the_three_directions_are_three_operators():
    """wall / freespace / periodic: A of direction d differs from the two others on the same input (else a sweep per direction shows nothing)"""
    c = H.case("mixed16")
    out = [c.A(d)(c.rhs) for d in range(3)]
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2])
    print("mixed16: A of direction 0 and of direction 2 are", "the same" if np.array_equal(out[0], out[2]) else "different", "on a random field")


def test_a_cap_of_100_restarts_gives_the_bits_of_no_cap():
    """max_restarts = 100 (PoissonSolverAMR) against 2^31 - 1 (how the device states 'no cap') where fewer than 100 restarts happen"""
    c = H.case("l012")
    a, ka, sa = _restated_solve(c, 0, max_restarts=100)
    b, kb, sb = _restated_solve(c, 0, max_restarts=H.UNBOUNDED)
    assert 1 <= sa["restarts"] < 100
    assert (ka, sa["restarts"]) == (kb, sb["restarts"]) and np.array_equal(a, b)


# ------------------------------------------------------------------ what the device sweeps need of their inputs

@pytest.mark.parametrize("name,M", [("mixed16", 8), ("l012", 12), ("l012_fast", 8)])
def test_the_sweeps_norms_rise_without_a_restart(name, M):
    for d in range(3):
        norms, first = _first_restart(H.case(name, d), d, M)
        print(f"{name}, direction {d}: norms {' '.join(f'{v:.2e}' for v in norms)}")
        assert first is None, (name, d, first)
        assert _rises(norms), (name, d, norms)


def test_direction_1_passes_the_refresh_without_a_restart_and_direction_0_restarts_in_pass_31():
    norms, first = _first_restart(H.case("l012"), 1, 52)
    assert first is None and _rises(norms)
    norms, first = _first_restart(H.case("l012"), 0, 34)
    assert first == 31, first


# ------------------------------------------------------------------ check 2: the step

def _step(c, solver, sequential=False, mutation=None, pres=None):
    return S.euler(c.vel, c.pres if pres is None else pres, c.h, c.dt, c.nu, c.advect(sequential), c.diffusion_rhs, solver, mutation)


@pytest.mark.parametrize("sequential", [False, True], ids=["order_independent", "sequential"])
@pytest.mark.parametrize("name", ["l012", "mixed16", "uniform_mixed"])
def test_step_is_the_oracles_bit_for_bit(name, sequential):
    c = H.case(name)
    v, its = c.oracle.advdiff_implicit(c.vel, c.pres, c.dt, c.nu, c.uinf, sequential, *TIGHT)
    got = _step(c, c.oracle_solver(*TIGHT), sequential)
    assert np.array_equal(got["vel"], v), np.abs(got["vel"] - v).max()
    assert np.array_equal(got["pres"], c.pres)
    assert all(i > 3 for i in its)
    if name == "l012":   # ... and with the restated solver behind it
        counts = []

        def restated(rhs, x0, direction):
            x, k, _ = _restated_solve(c, direction, rhs, x0)
            counts.append(k)
            return x

        got = _step(c, restated, sequential)
        assert np.array_equal(got["vel"], v) and counts == list(its)


# ------------------------------------------------------------------ the mutation catalogue of the step

def _returns_its_guess(rhs, x0, direction):
    """what a solve capped at max_iter = 0 returns"""
    return x0.copy()


def _moved(a, b):
    """largest change of any returned array, relative to that array's max"""
    worst, which = 0.0, None
    for k in ("vel", "tmpV", "pres"):
        if not np.array_equal(a[k].view(np.int64), b[k].view(np.int64)):
            m = np.abs(b[k]).max()
            d = max(np.abs(a[k] - b[k]).max() / (m if m > 0 else 1.0), np.finfo(float).tiny)
            if d > worst:
                worst, which = d, k
    return worst, which


def _not_applicable(c, mode, mu):
    if mu == "ih3_of_the_neighbour" and c.uniform:
        return "one spacing on a uniform grid: the neighbour's is the same number"
    if mode == "max_iter 0" and mu == "direction_0_face_rule":
        return "no operator is applied in a solve of no iterations"
    if mode == "max_iter 0" and mu == "added_to_the_next_component":
        return "every solution is zero: adding it anywhere changes nothing"
    return None


SEEN = {}


@pytest.mark.parametrize("name,mode", [("l012", "tight"), ("mixed16", "tight"), ("l012", "max_iter 0"), ("mixed16", "max_iter 0"),
                                       ("uniform_mixed", "max_iter 0"), ("grid1280", "max_iter 0")])
def test_every_wrong_step_changes_a_returned_array(name, mode):
    """On the inputs of tests/test_gpu_implicit_step.py: `tight` = the chained test (solves at 1e-12 / 1e-11), `max_iter 0` = the tests in
    which every solve returns its zero guess.  pres_not_zeroed and guess_left_out at `tight` also stay BELOW the 1e-6 x change bound of
    test_implicit_diffusion_solver: converged solves agree to that level from any guess."""
    c = H.case(name)
    solver = c.oracle_solver(*TIGHT) if mode == "tight" else _returns_its_guess
    true = _step(c, solver)
    change = np.abs(true["vel"] - c.vel).max()
    for mu in S.MUTATIONS:
        why = _not_applicable(c, mode, mu)
        if why:
            print(f"{name}, {mode}: {mu}: not applicable ({why})")
            continue
        got = _step(c, solver, mutation=mu)
        d, which = _moved(got, true)
        dv = np.abs(got["vel"] - true["vel"]).max()
        print(f"{name}, {mode}: {mu}: moves {which} by {d:.1e} of its max; vel by {dv / change:.1e} x the velocity change")
        assert which is not None, (name, mode, mu)
        SEEN.setdefault(mu, []).append((name, mode))
        if mode == "tight" and mu in ("pres_not_zeroed", "guess_left_out"):
            assert dv <= 1e-6 * change, (name, mu, dv, change)
            assert np.array_equal(got["pres"], true["pres"])


def test_every_wrong_step_is_seen():
    if set(SEEN) != set(S.MUTATIONS):   # run alone or with a selection
        test_every_wrong_step_changes_a_returned_array("l012", "tight")
    assert set(SEEN) == set(S.MUTATIONS), set(S.MUTATIONS) - set(SEEN)
