"""Every BiCGSTAB iteration of the device against tests/bicgstab_restatement.py (PoissonSolverAMR::solve, main.cpp:14404-14616, restated
from the reference alone and pinned to the oracle bit for bit by tests/test_bicgstab_restatement.py).  MI355X only (-m gpu), testing build.

cup3d_poisson_solve with tol = tol_rel = 0 never stops by 14601, so max_iter = m ends it after exactly m iterations; solves are
deterministic, so the sweep m = 0 .. M from identical uploads reads the solver's state after every iteration (cup3d_debug_solver_vector /
cup3d_debug_solver_state).  For every transition m -> m + 1 the DEVICE's own state m goes through one restated iteration:

  vector updates   phat, s, shat, z, q, qhat, y, x, r, rhat, w of state m + 1 are the restatement's BITS (zeros' signs included), with the
                   device's alpha, beta of state m and its omega of state m + 1.  Where the reference applies A or M^-1 the restatement is
                   handed the device's own product (checked below), so one wrong vector does not hide behind another.
  operator products  t = A what_m, v = A zhat_{m+1} -- on the refresh iterations also s, z, w and b - r -- are the oracle's lhs BIT FOR BIT.
                   bMeanConstraint 1: every cell but the corner cell against lhs(., 0); 2: the device's cells are lhs(., 0) + one constant,
                   bit for bit; the corner cell / the constant within the summation bound of the long-double sum(u h^3) of the device's u.
  block solves     zhat = M^-1 z, what = M^-1 w (refresh: shat, rhat too) inside the loop kernels against the exact 8^3 solve of the
                   device's own input: block_solve_exact.cg_bounds (block solvers 0, 2), 5e-14 max|z_exact| (1) -- and EQUAL to the
                   stand-alone cup3d_preconditioner on the same input (one cg_block / fdm_block behind both launches).
  dot products     each of the seven totals within gamma sum|a_i b_i| of the long-double dot of the device's vectors,
                   gamma = (N + 1) u / (1 - (N + 1) u), N cells, u = 2^-53: any order of summation obeys it; q.y, y.y where the host saw them.
  omega            inside the interval those bounds on q.y and y.y leave for 14493 (one more u for each of its two roundings).
  scalars          alpha, beta, r0r_prev, norm, min_norm, restarts, state, the x buffers and the count: reference_step2
                   (tests/test_solver_recurrences.py) of the device's seven totals, bit for bit.
  restart          a transition that ends in 14567-14593: r0 = r, rhat, w, what, t through the same operator and block-solve checks,
                   alpha = r0.r0 / (r0.w + eps) of the device's two totals, beta = omega = 0.
  init             state 0 is init(b, x0) by the same rules (once from a nonzero pressure).
  x_opt            pres after the solve capped at m is the logical x of the iteration with the smallest norm among 1 .. m, bit for bit;
                   every sweep asserts first that its norms are NOT monotone (else the snapshot is always the last iterate).

Which t: the loop kernels of a uniform grid form t = A what_m in the first loop of iteration m + 1, so state m holds an older t there;
where the LHS is a launch of its own state m holds it already (include/cup3d_hip_testing.h).  Per block, ONE of the device's two t
vectors (state m, state m + 1) must be the oracle's A what_m; that one is what the restated iteration consumes.

The operator is an object (class Poisson below: solve entry point, A, the block solve's centre coefficient, the stand-alone block solve,
the mean-constraint mode, the restart cap); tests/test_gpu_helmholtz_iteration.py runs the same checks on DiffusionSolver::solve.

Nothing here is a measured tolerance.  Worst observed ratios to the bounds are printed per sweep and recorded in tests/README.md."""
import ctypes as C

import numpy as np
import pytest

import bicgstab_cases as K
import bicgstab_restatement as R
import block_solve_exact as X
import cup3d_amd as cu
from cup3d_amd.capi import check, lib
from test_gpu_block_preconditioner import FDM_TOL, assert_block_cg
from test_solver_recurrences import KEYS, reference_step2

pytestmark = pytest.mark.gpu
LD = np.longdouble
f64 = np.float64
VEC = {n: i for i, n in enumerate(("phat", "rhat", "shat", "what", "zhat", "qhat", "s", "w", "z", "t", "v", "q", "r", "y", "x", "r0", "b", "x_opt"))}
UPDATED = ("phat", "s", "shat", "z", "q", "qhat", "y", "x", "r", "rhat", "w")


@pytest.fixture(scope="module", autouse=True)
def _device():
    cu.device_init(0)


class options:
    """debug options for the body of the with-statement; production behaviour behind it"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            check(lib().cup3d_debug_set_option(k.encode(), v))

    def __exit__(self, *a):
        for k in self.kw:
            check(lib().cup3d_debug_set_option(k.encode(), 0))


class Poisson:
    """What a sweep has to know of the operator it sweeps -- here PoissonSolverAMR::solve; tests/test_gpu_helmholtz_iteration.py has the
    DiffusionSolver's.  mc: the mean-constraint mode of the LHS; centre(c): the centre coefficient of the block solve; restart_cap: what
    io[11] must read; host_steps(k): does the host step omega in iteration k (check_sweep)."""
    restart_cap = 100

    def __init__(self, mc, block_solver):
        self.mc, self.block_solver = mc, block_solver
        self.label = f"bMeanConstraint {mc}, block solver {block_solver}"

    def sim(self, c, **kw):
        return cu.SimulationData(bMeanConstraint=self.mc, poissonTol=0.0, poissonTolRel=0.0, blockSolver=self.block_solver, **{**c.sim_kw, **kw})

    def solve(self, c, sim, max_iter):
        """the solve entry point with tol = tol_rel = 0, capped at max_iter"""
        p, r = sim.poisson_params(), cu.capi.PoissonResult()
        p.max_iter = max_iter
        check(lib().cup3d_poisson_solve(sim.handle, C.byref(p), C.byref(r)))
        return r

    def A(self, c, u, mc=None):
        return c.oracle.lhs(u, self.mc if mc is None else mc)

    def centre(self, c):
        return -6.0

    def precondition(self, c, sim):
        """the stand-alone block solve, in place on pres"""
        check(lib().cup3d_preconditioner(sim.handle, self.block_solver))

    def host_steps(self, k):
        return k % 50 == 0


def bits(a, b):
    """the same bits (signs of zeros included)"""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def blocks_equal(a, b):
    return (np.ascontiguousarray(a).view(np.int64) == np.ascontiguousarray(b).view(np.int64)).reshape(len(a), -1).all(axis=1)


def ld_dot(a, b):
    return np.sum(a.ravel().astype(LD) * b.ravel().astype(LD))


class Worst(dict):
    """worst observed ratio to each bound of a sweep"""

    def see(self, key, ratio):
        self[key] = max(self.get(key, 0.0), float(ratio))


def read_state(sim):
    io, totals = np.zeros(16), np.zeros(9)
    check(lib().cup3d_debug_solver_state(sim.handle, io, totals))
    st = {"io": io, "totals": totals, "pres": sim.download("pres")}
    for n, i in VEC.items():
        if n == "x_opt" and io[13] < 0:
            continue
        out = np.empty((sim.nblocks, 8, 8, 8))
        check(lib().cup3d_debug_solver_vector(sim.handle, i, out))
        st[n] = out
    return st


def sweep(c, op, M, stop=None):
    """the device's state after m = 0 .. M iterations, from identical uploads; stop(states): end the sweep early"""
    sim = op.sim(c)
    assert np.array_equal(sim.grid.tables[:, :5], c.oracle.tables[:, :5])
    states = []
    for m in range(M + 1):
        sim.upload("lhs", c.rhs)
        sim.upload("pres", c.x0)
        r = op.solve(c, sim, m)
        assert r.iterations == m
        states.append(read_state(sim))
        assert int(states[-1]["io"][14]) == m and int(states[-1]["io"][11]) == op.restart_cap
        if stop is not None and stop(states):
            break
    return sim, states


# ------------------------------------------------------------------ the operator products

def mean_bound(c, u):
    """(long-double sum(u h^3), the summation bound on the device's own total of it)"""
    return ld_dot(u, c.h3), K.gamma(u.size) * float(np.abs(u * c.h3).sum())


def find_constant(f, target, guess, reach=256):
    """the double within `reach` units in the last place of `guess` for which f(constant) is `target` bit for bit; None when there is none"""
    lo = hi = f64(guess)
    for _ in range(reach + 1):
        for cand in (lo, hi):
            if bits(f(cand), target):
                return cand
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    return None


def constant_of_mode_2(ref0, dev, b):
    """bMeanConstraint 2 (9314): dev = fl(ref0 + k) in every cell -- or fl(b - fl(ref0 + k)), the true residual -- for ONE double k.
    Every cell confines k to an interval (half a unit in the last place of each rounding); a double of their intersection that
    reproduces every bit of dev is returned with the intersection's width (k is known no better), None when there is none."""
    inner = dev.astype(LD) if b is None else b.astype(LD) - dev.astype(LD)
    half = np.spacing(np.abs(dev)).astype(LD) / 2
    if b is not None:
        half = half + np.spacing(np.abs(b) + np.abs(dev)).astype(LD) / 2
    lo, hi = (inner - half - ref0.astype(LD)).max(), (inner + half - ref0.astype(LD)).min()
    if lo > hi:
        return None
    k = find_constant((lambda k: ref0 + k) if b is None else (lambda k: b - (ref0 + k)), dev, f64((lo + hi) / 2))
    return None if k is None else (k, float(hi - lo))


def lhs_is_the_oracles(c, op, u, dev, what, worst, b=None):
    """per block (bool [nb]): dev is A u bit for bit -- or, with b, the true residual b - A u.  bMeanConstraint 1 and 2: outside the
    mean-constraint row against lhs(u, 0); the row itself (corner cell / the one constant added to every cell) is asserted, where the
    cells around it match, to lie within the summation bound of the long-double sum(u h^3), plus u for each rounding that follows."""
    post = (lambda a: a) if b is None else (lambda a: b - a)
    mc = op.mc
    if mc == 0 or mc > 2:
        return blocks_equal(post(op.A(c, u)), dev)
    total, bound = mean_bound(c, u)
    ref0 = op.A(c, u, 0)
    if mc == 1:
        ref0.ravel()[c.corner] = f64(total)
        ref = post(ref0)
        want = ref.ravel()[c.corner]
        got = dev.ravel()[c.corner]
        ref.ravel()[c.corner] = got
        ok = blocks_equal(ref, dev)
        if ok[c.corner // 512]:
            slack = bound + 2 * K.U * (abs(want) + abs(float(total)))
            worst.see("mean row / bound", abs(got - want) / slack if slack else 0.0)   # (slack 0: u = 0, the row is exactly 0)
            assert abs(got - want) <= slack, (what, got, want, slack)
        return ok
    assert np.ptp(c.h) == 0, "bMeanConstraint 2 is swept on uniform grids"
    h3 = f64(c.h[0]) * f64(c.h[0]) * f64(c.h[0])
    found = constant_of_mode_2(ref0, dev, b)
    if found is None:
        return np.zeros(len(dev), dtype=bool)
    k, width = found
    want = float(total) * h3
    slack = bound * h3 + 2 * K.U * abs(want) + width
    worst.see("mean row / bound", abs(k - want) / slack)
    assert abs(k - want) <= slack, (what, k, want, slack)
    return np.ones(len(dev), dtype=bool)


def assert_lhs(c, op, u, dev, what, worst, b=None):
    ok = lhs_is_the_oracles(c, op, u, dev, what, worst, b)
    assert ok.all(), f"{what}: not the oracle's lhs on blocks {np.where(~ok)[0][:8]}"


def assert_block_solve(c, op, sim, rhs, z, what, worst):
    """z = M^-1 rhs as the solver computed it: against the exact block solve, and equal to the stand-alone launch"""
    block_solver, centre = op.block_solver, op.centre(c)
    if block_solver == 1:
        zx = X.exact_block_solve(rhs, c.h)
        n = len(z)
        sk = X.skipped(rhs, c.h)
        assert (z[sk] == 0).all(), what
        d = np.abs(z - zx).reshape(n, -1).max(axis=1)
        m = np.abs(zx).reshape(n, -1).max(axis=1)
        if (~sk).any():
            worst.see("direct block solve / 5e-14 max|z|", (d[~sk] / (FDM_TOL * m[~sk])).max())
        bad = np.where(~sk & (d > FDM_TOL * m))[0]
        assert not len(bad), f"{what}: blocks {bad[:8]}: {(d[bad] / m[bad]).max():.3e} > {FDM_TOL}"
    else:
        rb, eb, _ = X.cg_bounds(rhs, c.h, centre)
        rn, _ = X.block_residual(z, rhs, c.h, centre)
        s = ~X.skipped(rhs, c.h)
        if s.any():
            worst.see("block CG residual / bound", (rn / rb)[s].max())
        assert_block_cg(z, rhs, c.h, centre, what)
    sim.upload("pres", rhs)
    op.precondition(c, sim)
    alone = sim.download("pres")
    assert bits(alone, z), f"{what}: the block solve inside the loop kernel is not the stand-alone one: {int((alone != z).sum())} cells differ"


class Replay:
    """A and M^-1 for the restated iteration: the device's own products, in the order the reference asks for them"""

    def __init__(self, outputs):
        self.outputs, self.inputs = list(outputs), []

    def __call__(self, u):
        self.inputs.append(u)
        out = self.outputs[len(self.inputs) - 1]
        return out(u) if callable(out) else out


def dot_bounds(pairs, totals, n_cells, what, worst):
    g = K.gamma(n_cells)
    for (name, a, b), t in zip(pairs, totals):
        exact, bound = ld_dot(a, b), g * float(np.abs(a * b).sum())
        worst.see("dot product / bound", abs(LD(t) - exact) / bound if bound else 0.0)
        assert abs(LD(t) - exact) <= bound, (what, name, t, float(exact), bound)


def omega_interval(q, y, n_cells):
    g = K.gamma(n_cells)
    qy, yy = ld_dot(q, y), ld_dot(y, y)
    e1, e2 = LD(g) * LD(np.abs(q * y).sum()), LD(g) * yy
    assert yy - e2 > 0
    corners = [(qy + s1 * e1) / (yy + s2 * e2 + LD(1e-100)) for s1 in (-1, 1) for s2 in (-1, 1)]
    lo, hi = min(corners), max(corners)
    return lo - 2 * K.U * abs(lo), hi + 2 * K.U * abs(hi), qy / yy


def recover_omega(S1):
    """after a restart omega is 0 again and, where the device stepped it, q.y and y.y are gone: the omega of r = q - omega y, from the cell
    with the largest |y| and a search of the doubles around it for the one that gives every bit of r"""
    q, y, r = S1["q"], S1["y"], S1["r"]
    j = int(np.argmax(np.abs(y)))
    guess = (q.ravel()[j] - r.ravel()[j]) / y.ravel()[j]
    return find_constant(lambda om: q - om * y, r, guess, reach=4096)


def scalars_of(io):
    return {k: (f64(io[i]) if i < 9 else int(io[i])) for i, k in enumerate(KEYS)}


def check_init(c, op, sim, S0, worst):
    what = f"{c.name}, init"
    mc = op.mc
    b = c.rhs.copy()
    if c.zero_corner(mc) is not None:
        b.ravel()[c.corner] = 0.0
    assert bits(S0["b"], b) and bits(S0["x"], c.x0) and bits(S0["pres"], c.x0)
    assert_lhs(c, op, c.x0, S0["r0"], what + ": r0 = b - A x0", worst, b=b)
    assert bits(S0["r"], S0["r0"])
    assert_block_solve(c, op, sim, S0["r0"], S0["rhat"], what + ": rhat", worst)
    assert_lhs(c, op, S0["rhat"], S0["w"], what + ": w = A rhat", worst)
    assert_block_solve(c, op, sim, S0["w"], S0["what"], what + ": what", worst)
    assert_lhs(c, op, S0["what"], S0["t"], what + ": t = A what", worst)
    t0, t1 = f64(S0["totals"][0]), f64(S0["totals"][1])
    dot_bounds([("r0.r0", S0["r0"], S0["r0"]), ("r0.w", S0["r0"], S0["w"])], (t0, t1), c.rhs.size, what, worst)
    sc = scalars_of(S0["io"])
    want = dict(alpha=t0 / (t1 + R.EPS), beta=f64(0), omega=f64(0), r0r_prev=t0, norm=np.sqrt(t0), init_norm=np.sqrt(t0), min_norm=f64(1e50))
    for k, v in want.items():
        assert sc[k].tobytes() == f64(v).tobytes(), (what, k, sc[k], v)
    assert (sc["restarts"], sc["xcur"], sc["xopt"], sc["iter"], sc["state"]) == (0, 0, -1, 0, 0)


def check_transition(c, op, sim, S0, S1, k, worst):
    what = f"{c.name}, {op.label}, iteration {k} -> {k + 1}"
    mc = op.mc
    refresh = k % 50 == 0
    restarted = bool(S1["io"][15])
    n_cells = c.rhs.size
    sc0, sc1 = scalars_of(S0["io"]), scalars_of(S1["io"])
    # ---- the t this iteration consumes: A what_m, from whichever of the device's two t vectors holds it (module docstring)
    t_m = S0["t"]
    if not refresh:
        at_end = lhs_is_the_oracles(c, op, S0["what"], S0["t"], what + ": t of state m", worst)
        if restarted and not at_end.all():
            # the restart wrote its own t = A what over the one the first loop formed: A what_m is nowhere on the device any more, and the
            # oracle's (the same bits wherever the device's can be seen) stands in -- without a mean row to guess (bMeanConstraint 0, 3)
            assert mc == 0 or mc > 2
            t_m = np.where(at_end.reshape(-1, 1, 1, 1), S0["t"], op.A(c, S0["what"]))
        else:
            in_loop = lhs_is_the_oracles(c, op, S0["what"], S1["t"], what + ": t of state m + 1", worst)
            assert (at_end | in_loop).all(), f"{what}: t = A what_m is in neither of the device's t vectors on blocks {np.where(~(at_end | in_loop))[0][:8]}"
            t_m = np.where(at_end.reshape(-1, 1, 1, 1), S0["t"], S1["t"])
    # ---- the omega the device used
    if restarted:
        if np.isfinite(S1["totals"][7]):
            omega = f64(S1["totals"][7]) / (f64(S1["totals"][8]) + R.EPS)
        else:
            omega = recover_omega(S1)
            assert omega is not None, f"{what}: no omega gives the device's r = q - omega y"
    else:
        omega = sc1["omega"]
    # ---- one restated iteration of the device's state m, its A and M^-1 answered by the device's own products
    st = {n: S0[n] for n in R.VECTORS}
    st.update(t=t_m, x_opt=S0.get("x_opt", np.zeros_like(c.rhs)), alpha=sc0["alpha"], beta=sc0["beta"], omega=sc0["omega"], r0r_prev=sc0["r0r_prev"],
              norm=sc0["norm"], init_norm=sc0["init_norm"], min_norm=sc0["min_norm"], restarts=sc0["restarts"], useXopt=sc0["xopt"] >= 0)
    true_resid = []   # the refresh's r = b - A x: the restatement gets A x as the oracle has it; the device's r is judged below
    if refresh:
        def lhs_of_x(u):
            true_resid.append(u)
            return op.A(c, u, mc if (mc == 0 or mc > 2) else 0)
        a_out = [S1["s"], S1["z"], S1["v"], lhs_of_x, S1["w"], S1["t"]]
        m_out = [S1["shat"], S1["zhat"], S1["rhat"], S1["what"]]
    else:
        a_out = [S1["v"], S1["t"]]
        m_out = [S1["zhat"], S1["what"]]
    if restarted:    # 14572-14587 overwrite rhat, w, what, t: what the device holds is the restart's
        a_out = a_out[:-1] + [S1["t"], S1["w"], S1["t"]]
        m_out = m_out + [S1["rhat"], S1["what"]]
    A, M = Replay(a_out), Replay(m_out)
    given = {"omega": omega, "seven": tuple(S1["totals"][:7])}
    if restarted:
        # r0.r and r0.w of 14546 are gone (the restart's two totals took their place): the long-double values decide the breakdown test,
        # which the restart the device reports must agree with
        given["seven"] = (float(ld_dot(S0["r0"], S1["r"])), 0.0) + tuple(S1["totals"][2:7])
        given["restart"] = tuple(S1["totals"][:2])
    with np.errstate(all="ignore"):
        new = R.iteration(st, k, A, M, dots="longdouble", max_restarts=sc0["max_restarts"], given=given)
    assert new["restarted"] == restarted, f"{what}: the device {'restarted' if restarted else 'went on'}, the breakdown test of its own vectors says otherwise"
    # ---- vector updates, bit for bit
    names = [n for n in UPDATED if not (restarted and n in ("rhat", "w"))] + (["r0"] if restarted else [])
    for n in names:
        if n == "r" and refresh and mc in (1, 2):
            assert_lhs(c, op, true_resid[0], S1["r"], what + ": r = b - A x", worst, b=S0["b"])
            assert bits(true_resid[0], S1["x"])
            continue
        if not bits(new[n], S1[n]):
            d = np.abs(new[n] - S1[n])
            raise AssertionError(f"{what}: {n} differs from the restated update in {int((new[n] != S1[n]).sum())} cells, max {d.max():.3e} "
                                 f"({d.max() / max(np.abs(S1[n]).max(), 1e-300) / K.U:.1f} x 2^-53 of max|{n}|), first block {int(np.argmax(d)) // 512}")
    assert bits(S1["r0"], S1["r"] if restarted else S0["r0"]) and bits(S1["b"], S0["b"])
    # ---- operator products and block solves on the device's own vectors
    assert_lhs(c, op, S1["zhat"], S1["v"], what + ": v = A zhat", worst)
    assert_block_solve(c, op, sim, S1["z"], S1["zhat"], what + ": zhat", worst)
    if refresh:
        assert_lhs(c, op, S1["phat"], S1["s"], what + ": s = A phat", worst)
        assert_block_solve(c, op, sim, S1["s"], S1["shat"], what + ": shat", worst)
        assert_lhs(c, op, S1["shat"], S1["z"], what + ": z = A shat", worst)
    if refresh or restarted:
        assert_block_solve(c, op, sim, S1["r"], S1["rhat"], what + ": rhat", worst)
        assert_lhs(c, op, S1["rhat"], S1["w"], what + ": w = A rhat", worst)
    assert_block_solve(c, op, sim, S1["w"], S1["what"], what + ": what", worst)
    if restarted:
        assert_lhs(c, op, S1["what"], S1["t"], what + ": t = A what after the restart", worst)
    # ---- dot products, omega
    r0 = S0["r0"]
    seven = [("r0.r", r0, S1["r"]), ("r0.w", r0, S1["w"]), ("r0.s", r0, S1["s"]), ("r0.z", r0, S1["z"]), ("r.r", S1["r"], S1["r"]), ("r0.r0", r0, r0),
             ("r.r", S1["r"], S1["r"])]
    if restarted:
        dot_bounds(seven[2:] + [("r0.r0 of the restart", S1["r0"], S1["r0"]), ("r0.w of the restart", S1["r0"], S1["w"])],
                   tuple(S1["totals"][2:7]) + tuple(S1["totals"][:2]), n_cells, what, worst)
    else:
        dot_bounds(seven, S1["totals"][:7], n_cells, what, worst)
    if np.isfinite(S1["totals"][7]):
        dot_bounds([("q.y", S1["q"], S1["y"]), ("y.y", S1["y"], S1["y"])], S1["totals"][7:9], n_cells, what, worst)
        assert (f64(S1["totals"][7]) / (f64(S1["totals"][8]) + R.EPS)).tobytes() == f64(omega).tobytes(), what
    lo, hi, mid = omega_interval(S1["q"], S1["y"], n_cells)
    worst.see("omega / interval", abs(LD(omega) - mid) / max(hi - mid, mid - lo))
    assert lo <= LD(omega) <= hi, (what, omega, float(lo), float(hi))
    # ---- scalars
    if not restarted:
        ref = reference_step2(dict(sc0, omega=f64(omega)), S1["totals"][:7])
        for key in KEYS:
            a, b = ref[key], sc1[key]
            assert (int(a) == int(b)) if isinstance(b, int) else (f64(a).tobytes() == f64(b).tobytes()), (what, key, a, b)
    else:
        t0, t1 = f64(S1["totals"][0]), f64(S1["totals"][1])
        norm = np.sqrt(f64(S1["totals"][6]))
        want = dict(alpha=t0 / (t1 + R.EPS), beta=f64(0), omega=f64(0), r0r_prev=t0, norm=norm, min_norm=min(norm, sc0["min_norm"]))
        for key, v in want.items():
            assert sc1[key].tobytes() == f64(v).tobytes(), (what, key, sc1[key], v)
        assert (sc1["restarts"], sc1["iter"], sc1["state"]) == (sc0["restarts"] + 1, k + 1, 0)


def sweep_over_ranks(c, op, M, nranks):
    """the same sweep on `nranks` thread ranks of the in-process communicator; every rank's vectors gathered into the one-rank slot
    order, scalars and (all-reduced) totals the same bits on every rank.  A uniform grid is cut by the library (rank = r of nranks), a
    multi-level mesh into contiguous ranges of its block order (rank views).  Returns a one-rank sim for the stand-alone block solves."""
    from test_gpu_multirank import VirtualComm, run_ranks
    o = c.oracle
    states = []
    with VirtualComm(nranks):
        if "leaves" in c.sim_kw:
            kw = c.sim_kw
            mesh = cu.operators.Grid((kw["bpdx"], kw["bpdy"], kw["bpdz"]), kw["levelMax"], 0, kw["extent"], (kw["BC_x"], kw["BC_y"], kw["BC_z"]), leaves=kw["leaves"])
            assert np.array_equal(mesh.tables, o.tables)
            owner = (np.arange(o.nb) * nranks // o.nb).astype(np.int32)
            views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
            sims = [op.sim(c, view=v, leaves=None) for v in views]
            mine = [v.global_slot[:v.nlocal] for v in views]
            uploads = [(c.rhs[mine[r]], c.x0[mine[r]]) for r in range(nranks)]

            def gather(parts):
                out = np.zeros_like(c.rhs)
                for r in range(nranks):
                    out[mine[r]] = parts[r]
                return out
        else:
            views = None
            sims = [op.sim(c, rank=r, nranks=nranks) for r in range(nranks)]
            rhs_g, x0_g = o.to_global(c.rhs), o.to_global(c.x0)
            uploads = [(s.grid.to_blocks(rhs_g), s.grid.to_blocks(x0_g)) for s in sims]

            def gather(parts):
                g = np.zeros_like(rhs_g)
                for r, s in enumerate(sims):
                    s.grid.scatter_to_global(parts[r], g)
                return o.to_blocks(g)
        assert sum(s.nblocks for s in sims) == o.nb and all(s.nblocks for s in sims)
        for m in range(M + 1):
            per_rank = [None] * nranks

            def rank(r):
                s = sims[r]
                s.upload("lhs", uploads[r][0])
                s.upload("pres", uploads[r][1])
                res = op.solve(c, s, m)
                assert res.iterations == m
                per_rank[r] = read_state(s)

            run_ranks(rank, nranks)
            st = {"io": per_rank[0]["io"], "totals": per_rank[0]["totals"]}
            for r in range(1, nranks):
                assert bits(per_rank[r]["io"], st["io"]) and bits(per_rank[r]["totals"][:7], st["totals"][:7]), f"rank {r}: other scalars than rank 0"
            for n in [n for n in per_rank[0] if n not in ("io", "totals")]:
                st[n] = gather([per_rank[r][n] for r in range(nranks)])
            states.append(st)
        del sims, views
    return op.sim(c), states


def check_sweep(c, op, M, stop=None, need_restart=False, host_steps=None, nranks=1, norms_must_rise=True):
    """host_steps(k): does the host step omega in iteration k (a host-driven iteration; default: the operator's own rule) -- where it does,
    q.y and y.y are reported; asserted, so that a debug option that silently did nothing cannot leave a sweep on the production path.
    norms_must_rise=False: a sweep too short for its norms to rise (the x_opt snapshot is then the last iterate throughout, and is checked
    as that); every sweep of the Poisson solver keeps the precondition."""
    host_steps = host_steps or op.host_steps
    worst = Worst()
    sim, states = sweep(c, op, M, stop) if nranks == 1 else sweep_over_ranks(c, op, M, nranks)
    for k, s in enumerate(states[1:]):
        assert bool(np.isfinite(s["totals"][7])) == bool(host_steps(k)), f"iteration {k}: {'fused' if host_steps(k) else 'host-driven'}, not as this sweep expects"
    norms = [float(s["io"][4]) for s in states]
    print(f"{c.name}, {op.label}: norms {' '.join(f'{v:.3e}' for v in norms[:10])}{' ...' if len(norms) > 10 else ''}")
    if norms_must_rise:
        assert any(b >= a for a, b in zip(norms[1:], norms[2:])), "precondition: the norms of this sweep are monotone -- choose another right-hand side"
    restarts = [m for m, s in enumerate(states) if s["io"][15]]
    assert bool(restarts) == need_restart, (restarts, need_restart)
    check_init(c, op, sim, states[0], worst)
    for k in range(len(states) - 1):
        check_transition(c, op, sim, states[k], states[k + 1], k, worst)
    # x_opt: pres after the solve capped at m = the logical x of the first iteration with the smallest norm among 1 .. m
    differs = 0
    for m in range(1, len(states)):
        best = 1 + int(np.argmin(norms[1:m + 1]))
        assert bits(states[m]["pres"], states[best]["x"]), f"pres after {m} iterations is not the x of iteration {best}"
        assert bits(states[m]["x_opt"], states[best]["x"])
        differs += best != m
    assert differs > 0 or not norms_must_rise
    print(f"    worst ratios to the bounds over {len(states) - 1} transitions: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert all(v <= 1 for v in worst.values())
    return states


# ------------------------------------------------------------------ the cases

@pytest.mark.parametrize("mc", [0, 1])
@pytest.mark.parametrize("block_solver", [0, 1, 2])
@pytest.mark.parametrize("name", ["wall16", "pwp", "periodic_112"])
def test_eight_iterations_on_small_uniform_grids(name, block_solver, mc):
    """cases 1, 3, 4: 16^3 all-wall (8 blocks, three domain faces each), (2,1,1) level 1 periodic / wall / periodic (periodic neighbour
    slots), (1,1,2) level 0 all periodic (a block that is its own neighbour); every block solver"""
    check_sweep(K.case(name), Poisson(mc, block_solver), 8)


@pytest.mark.parametrize("mc", [0, 1, 2, 3])
def test_fifty_two_iterations_across_the_refresh(mc):
    """case 2: 32^3 all-wall, 64 blocks (interior, face, edge, corner): iteration 1 (k = 0, the refresh form), the fused runs, and the
    hand-over k = 49 -> 50 -> 51 into and out of k_refresh; all four bMeanConstraint modes.  No restart through iteration 52 on the
    oracle (the seed's choice, bicgstab_cases.py) nor on the device (asserted)."""
    check_sweep(K.case("wall32"), Poisson(mc, 0), 52)


@pytest.mark.parametrize("block_solver", [1, 2])
def test_fifty_two_iterations_with_the_other_block_solvers(block_solver):
    """case 2 with the direct block solve (its every-50th iteration is host-driven) and the reference's association of the block CG"""
    check_sweep(K.case("wall32"), Poisson(1, block_solver), 52)


@pytest.mark.parametrize("opts", [dict(loop1_five_waves=1), dict(loop1_five_waves=2), dict(loop2_five_waves=1), dict(loop2_five_waves=2),
                                  dict(no_fuse=1), dict(no_fuse_lhs=1)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_every_form_of_the_loop_kernels(opts):
    """the forms `loop1_five_waves` / `loop2_five_waves` 1 / 2 select (k_loop1_cg_w5 / k_loop1_cg, k_loop2_cg_w5 / k_loop2_cg_w4), the
    plain k_loop1 / k_loop2 path (`no_fuse`) and the fused kernels with the LHS as a launch of its own (`no_fuse_lhs`): 16^3, 8 iterations"""
    with options(**opts):
        check_sweep(K.case("wall16"), Poisson(1, 0), 8, host_steps=(lambda k: True) if "no_fuse" in opts else (lambda k: k % 50 == 0))


def test_the_refresh_launch_by_launch():
    """`no_fuse_refresh`: the every-50th iteration as sixteen launches instead of k_refresh, across k = 50"""
    with options(no_fuse_refresh=1):
        check_sweep(K.case("wall32"), Poisson(1, 0), 52)


@pytest.mark.parametrize("mc", [0, 1])
@pytest.mark.parametrize("fuse_lhs_ml", [0, 1])
def test_eight_iterations_on_a_multi_level_mesh(mc, fuse_lhs_ml):
    """case 5: synthetic_l012 -- the LHS (ghost slabs, flux correction) is a launch of its own between the loops; with `fuse_lhs_ml` the
    blocks without a coarse/fine face form theirs inside the loop kernels and only the interface blocks keep the launch"""
    with options(fuse_lhs_ml=fuse_lhs_ml):
        check_sweep(K.case("synthetic_l012"), Poisson(mc, 0), 8)


def test_init_from_a_nonzero_pressure():
    check_sweep(K.with_x0(K.case("wall16"), 12), Poisson(0, 0), 8)


@pytest.mark.parametrize("opts", [dict(), dict(no_fuse=1)], ids=["fused", "no_fuse"])
def test_a_transition_that_restarts(opts):
    """case 6: the all-wall Taylor-Green right-hand side of step 21 at level 1 (built with the oracle's pressure_rhs), bMeanConstraint 0:
    swept to the device's first restart + 2.  On the fused path the restart is reported one iteration after the host enqueued the next."""
    with options(**opts):
        states = check_sweep(K.case("tg_restart"), Poisson(0, 0), 120, stop=lambda s: len(s) >= 3 and bool(s[-3]["io"][15]), need_restart=True,
                             host_steps=(lambda k: True) if "no_fuse" in opts else (lambda k: k % 50 == 0))
    first = next(m for m, s in enumerate(states) if s["io"][15])
    print(f"    first restart at the end of iteration {first}")
    assert len(states) == first + 3


@pytest.mark.parametrize("mc", [0, 1])
def test_four_iterations_over_two_ranks(mc):
    """case 7: 32^3 over two thread ranks (the in-process communicator): faces towards the other rank from the halo slabs, launches split
    into inner and boundary blocks, totals all-reduced before the scalars are stepped.  Per-rank vectors gathered to the one-rank
    restatement; dot products and scalars against the all-reduced totals.  (The Taylor-Green right-hand side: bicgstab_cases.py says why.)"""
    check_sweep(K.case("tg32"), Poisson(mc, 0), 4, nranks=2)
