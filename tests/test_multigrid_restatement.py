"""tests/multigrid_restatement.py -- the dense NumPy statement of one V-cycle that tests/test_gpu_multigrid_cycle.py holds the device to --
made trustworthy WITHOUT a device:
  * it is a contraction for the operator the reference pins (the oracle's A, uniform and multi-level);
  * it is linear to the last bit under scaling by powers of two, and its float64 and longdouble evaluations agree to rounding;
  * every input the GPU tests use can tell it from ten deliberately wrong cycles by more than 1e6 x the GPU tests' tolerance.
"""
import numpy as np
import pytest

import multigrid_cases as K
import multigrid_restatement as R
import oracle_lib as O

# total residual fall over six cycles as recorded in the docstrings of the two tests below
RECORDED_FALL = {"uniform": 5.85e-6, "l012_wall": 1.07e-4}


def _six_cycles(A, V, xstar):
    b = A(xstar)
    x = np.zeros_like(b)
    norms = [np.linalg.norm(b)]
    for _ in range(6):
        x = x + V(b - A(x))
        norms.append(np.linalg.norm(b - A(x)))
    return [norms[i + 1] / norms[i] for i in range(6)], norms[6] / norms[0]


def _assert_contraction(what, ratios, fall, recorded):
    print(f"{what}: residual ratios of six cycles {[f'{v:.3f}' for v in ratios]}, total fall {fall:.2e} (recorded {recorded:.1e})")
    assert all(v < 1 for v in ratios), ratios
    assert fall <= 2 * recorded


def test_cycle_contracts_for_the_oracles_operator_uniform():
    """x <- x + V(b - A x) with A = the oracle's ComputeLHS (mean constraint 0) on (1,1,1) level 2, walls, b = A x* for a random x*: the
    residual falls in every cycle.  Recorded per-cycle ratios: 0.004 0.052 0.120 0.461 0.697 0.733, total 5.85e-6 (the first cycles
    take out what the smoother and the coarse levels see; then the slowest mode of a V(2,2) with piecewise-constant transfers remains).
    Asserted: every ratio < 1, and the total fall at most TWICE the recorded one -- the late ratios
    depend on how much of the slowest mode the random x* happens to hold, which another generator or summation order in NumPy shifts by
    tens of per cent; a cycle that is structurally wrong (tests below) loses orders of magnitude or diverges."""
    bpd, level, bc = (1, 1, 1), 2, ("wall", "wall", "wall")
    o = O.OracleGrid(bpd, level + 1, level, K.EXT, bc)
    NX, NY, NZ = o.ncell
    xs = np.random.default_rng(1).uniform(-1, 1, (NZ, NY, NX))
    ratios, fall = _six_cycles(lambda x: o.to_global(o.lhs(o.to_blocks(x), 0)), lambda r: R.vcycle_uniform(r, bpd, level, bc, o.h), xs)
    _assert_contraction("(1,1,1) level 2 wall", ratios, fall, RECORDED_FALL["uniform"])


def test_cycle_contracts_for_the_oracles_operator_multilevel():
    """The same on the three-level mesh l012_wall with the multi-level oracle's A (coarse/fine interpolation and flux matching included,
    which the cycle ignores: it only has to be close).  Recorded ratios: 0.032 0.185 0.260 0.345 0.415 0.486, total 1.07e-4; asserted as
    above."""
    m, M = K.oracle_mesh("l012_wall")
    xs = np.random.default_rng(1).uniform(-1, 1, (m.nb, 8, 8, 8))
    ratios, fall = _six_cycles(lambda x: m.lhs(x, 0), lambda r: R.vcycle_blocks(M, r), xs)
    _assert_contraction("l012_wall", ratios, fall, RECORDED_FALL["l012_wall"])


def test_level_sizes_are_the_oracles():
    for bpd, level, bc in K.UNIFORM.values():
        assert K.EXT / (8 * (max(bpd) << level)) == O.OracleGrid(bpd, level + 1, level, K.EXT, bc).h
    for name in K.MESHES:
        m, M = K.oracle_mesh(name)
        assert all(m.h(b) == M.h0 * 2.0 ** -int(m.tables[b, 0]) for b in range(m.nb))
        assert sum(int(l.sum()) for l in M.leaf) == m.nb and M.nlev == 3 and sum(int(n.sum()) for n in M.node) > m.nb


@pytest.mark.parametrize("case", ["three_levels_211", "box_321", "one_level_8_blocks", "l012_periodic"])
def test_scaling_is_exact_and_the_precisions_agree(case):
    """V(2^k r) == 2^k V(r) bit for bit (every operation is linear and IEEE, the constants 1/6, 1/h, 6, h and the cell count are untouched
    by the scale), and float64 against longdouble to rounding: below 8 eps max|z| (3e-16 ... 1.6e-15 seen)."""
    if case in K.UNIFORM:
        r, (z, zl) = K.restated_uniform(case, "random")
        bpd, level, bc = K.UNIFORM[case]
        V = lambda v: R.vcycle_uniform(v, bpd, level, bc, K.EXT / (8 * (max(bpd) << level)))
    else:
        m, M = K.oracle_mesh(case)
        r = K.mesh_input(m.nb)
        z, zl = K.restated((case, 2, 2), lambda dt: R.vcycle_blocks(M, r, dtype=dt))
        V = lambda v: R.vcycle_blocks(M, v)
    for k in (-3, 5):
        assert np.array_equal(V(r * 2.0 ** k), z * 2.0 ** k), k
    d = float(np.abs(z - zl).max() / np.abs(zl).max())
    print(f"{case}: float64 against longdouble {d:.2e} of max|z|")
    assert d <= 8 * K.EPS


def _not_applicable(mutation, levels, uniform, bc, nblocks0):
    """Why a case cannot see a mutation (None: it must)."""
    if levels == 1 and mutation in ("restrict_average", "keep_mean", "prolong_mirrored_octant", "coarse_h_not_doubled"):
        return "a one-level hierarchy has no coarse level"
    if uniform and mutation.startswith("cf_ghosts"):
        return "a uniform grid has no coarse/fine face"
    if mutation == "domain_ghost_zero":
        if all(b == "periodic" for b in bc):
            return "no domain face: every direction is periodic"
        if levels == 1 and nblocks0 == 1:
            return "one launch from zero: its frozen ghosts are the zero guess whatever the rule"
    return None


SEEN = {}


def _catalogue(what, V, z, zl, levels, uniform, bc, nblocks0):
    tol = K.tolerance(z, zl)
    for mutation in R.MUTATIONS:
        why = _not_applicable(mutation, levels, uniform, bc, nblocks0)
        if why:
            print(f"{what}: {mutation}: not applicable ({why})")
            continue
        moved = float(np.abs(V(mutation) - z).max())
        print(f"{what}: {mutation}: moves the result by {moved / tol:.1e} x the tolerance")
        assert moved > K.MUTATION_FACTOR * tol, (what, mutation, moved / tol)
        SEEN[mutation] = SEEN.get(mutation, 0) + 1


def _uniform_configs():
    for case in K.UNIFORM:
        for kind in K.INPUTS:
            yield case, kind, 2, 2
        if case in K.SCHEDULE_CASES:
            for nu, sw in K.SCHEDULES:
                yield case, "random", nu, sw
    yield "ranks", "random", 2, 2


@pytest.mark.parametrize("case,kind,launches,sweeps", list(_uniform_configs()))
def test_mutations_are_visible_uniform(case, kind, launches, sweeps):
    """Every (case, input, schedule) of the GPU tests: each wrong cycle of multigrid_restatement.MUTATIONS that the case can see at all moves
    the float64 result by more than 1e6 x the tolerance the device is held to.  A condition on the INPUTS."""
    bpd, level, bc = K.RANKS_CASE if case == "ranks" else K.UNIFORM[case]
    kw = dict(depth=2, coarsest=(16, 4)) if case == "ranks" else {}
    r, (z, zl) = K.restated_uniform(case, kind, launches, sweeps, **kw)
    levels = kw.get("depth", level + 1)
    nblocks0 = bpd[0] * bpd[1] * bpd[2] << (3 * (level + 1 - levels))
    h = K.EXT / (8 * (max(bpd) << level))
    _catalogue(f"{case}, {kind}, {launches} x {sweeps}", lambda mu: R.vcycle_uniform(r, bpd, level, bc, h, launches=launches, sweeps=sweeps, mutation=mu, **kw),
               z, zl, levels, True, bc, nblocks0)


@pytest.mark.parametrize("launches,sweeps", [(2, 2), (1, 3)])
@pytest.mark.parametrize("name", K.MESHES)
def test_mutations_are_visible_multilevel(name, launches, sweeps):
    m, M = K.oracle_mesh(name)
    r = K.mesh_input(m.nb)
    z, zl = K.restated((name, launches, sweeps), lambda dt: R.vcycle_blocks(M, r, dtype=dt, launches=launches, sweeps=sweeps))
    _catalogue(f"{name}, {launches} x {sweeps}", lambda mu: R.vcycle_blocks(M, r, launches=launches, sweeps=sweeps, mutation=mu), z, zl, M.nlev, False,
               K.mesh_case(name)[2], int(M.node[0].size))


def test_every_mutation_is_seen_by_some_case():
    """(after the two catalogues above, in file order) no rule of the cycle is left to cases that cannot see it"""
    if set(SEEN) != set(R.MUTATIONS):   # run alone or with a selection: one case of each kind sees all ten
        test_mutations_are_visible_uniform("two_levels", "random", 2, 2)
        test_mutations_are_visible_multilevel("l012_wall", 2, 2)
    assert set(SEEN) == set(R.MUTATIONS), set(R.MUTATIONS) - set(SEEN)
