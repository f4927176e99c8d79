"""cup3d_compute_dissipation and cup3d_fix_mass_flux on a grid spread over ranks: the ranks are host threads, the in-process communicator
(cup3d_debug_virtual_comm) stands in for RCCL, and every ghost cell that is not shipped is poisoned with NaN (`poison_ghosts`), as in
tests/test_gpu_multirank.py.  MI355X only (-m gpu).

  * a rank's per-block rows are bit for bit the rows of the same blocks on one rank (= the restatement's): the pres ghosts parked behind
    the vel ghosts in the slab buffer, the ghost-block exchange of rank views, the coarse-fine ghosts across ranks;
  * the totals are bit for bit the restatement's per-rank totals (the rank's rows added from 0.0 in its slot order) combined in the
    all-reduce's association.  The virtual communicator adds the ranks' operands in RANK ORDER (k_vreduce, comm.hip): r0 + r1 on two
    ranks, (r0 + r1) + r2 on three -- asserted below; RCCL's own association is RCCL's.
  * FixMassFlux: each rank divides its sum by the volume BEFORE the all-reduce (12214, 12224); given the all-reduced mean every bit of
    vel on every rank is the restatement's."""
import numpy as np
import pytest

import cup3d_amd as cu
import dissipation_cases as D
import dissipation_restatement as R
import labs_ranks_cases as LR
from cup3d_amd.capi import check, lib
from test_gpu_multirank import VirtualComm, run_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


@pytest.fixture(scope="module", autouse=True)
def _device_and_poison():
    cu.device_init(0)
    check(lib().cup3d_debug_set_option(b"poison_ghosts", 1))
    yield
    check(lib().cup3d_debug_set_option(b"poison_ghosts", 0))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def rank_sims(c, nranks, kind, **kw):
    """([SimulationData per rank], [global slots of the rank's local blocks, in its slot order])"""
    if c.uniform_level is not None:
        sims = [cu.SimulationData(rank=r, nranks=nranks, **c.sim_kwargs, **kw) for r in range(nranks)]
        slot_of_z = {int(z): i for i, z in enumerate(c.tables[:, 1])}
        return sims, [np.array([slot_of_z[int(z)] for z in s.grid.tables[:, 1]]) for s in sims], None
    mesh = cu.operators.Grid(c.bpd, c.lmax, 0, D.EXT, c.bc, leaves=c.leaves)
    owner = LR.owners(c.nb, kind, nranks, 11)
    views = [mesh.rank_view(owner, r, nranks) for r in range(nranks)]
    k = {key: v for key, v in c.sim_kwargs.items() if key not in ("leaves",)}
    sims = [cu.SimulationData(view=views[r], **k, **kw) for r in range(nranks)]
    return sims, [np.array(v.global_slot[:v.nlocal]) for v in views], views


def in_rank_order(values):
    t = values[0]
    for v in values[1:]:
        t = t + v
    return t


@pytest.mark.parametrize("name,nranks,kind", [("uniform_222", 2, "ranges"), ("l012_wall", 3, "scattered")])
def test_rows_and_totals_over_ranks(name, nranks, kind):
    c = D.case(name)
    want_rows, _, _ = D.expected(name)
    one = cu.SimulationData(**c.sim_kwargs)
    one.upload("vel", c.vel); one.upload("pres", c.pres)
    if c.chi is not None:
        one.upload("chi", c.chi)
    cu.ComputeDissipation(one).compute(block_sums=True)
    one_rows = one.diagnostics["block_sums"]
    assert np.array_equal(bits(one_rows[:, :19]), bits(want_rows[:, :19]))
    got = [None] * nranks
    with VirtualComm(nranks):
        sims, mine, views = rank_sims(c, nranks, kind)
        assert sorted(np.concatenate(mine).tolist()) == list(range(c.nb)) and all(len(m) for m in mine)

        def rank(r):
            s = sims[r]
            s.upload("vel", c.vel[mine[r]]); s.upload("pres", c.pres[mine[r]])
            if c.chi is not None:
                s.upload("chi", c.chi[mine[r]])
            q = cu.ComputeDissipation(s).compute(block_sums=True).copy()
            q2 = cu.ComputeDissipation(s).compute(block_sums=True)
            assert np.array_equal(bits(q), bits(q2))
            got[r] = (q, s.diagnostics["block_sums"].copy())

        run_ranks(rank, nranks)
        del sims, views
    for r in range(nranks):
        assert np.array_equal(bits(got[r][1]), bits(one_rows[mine[r]])), r                  # every column: the same device arithmetic
        assert np.array_equal(bits(got[r][0]), bits(got[0][0]))                             # every rank holds the same totals
    per_rank = [np.array(R.totals(want_rows[mine[r]])) for r in range(nranks)]
    want = in_rank_order(per_rank)
    assert np.array_equal(bits(got[0][0][:19]), bits(want[:19]))
    own = in_rank_order([np.array(R.totals(got[r][1])) for r in range(nranks)])
    assert np.array_equal(bits(got[0][0]), bits(own))
    if nranks == 3:   # the association is the rank order, and on this case it can be told from r0 + (r1 + r2)
        other = per_rank[0] + (per_rank[1] + per_rank[2])
        assert not np.array_equal(bits(other[:19]), bits(want[:19]))


@pytest.mark.parametrize("name,nranks,kind", [("uniform_222", 2, "ranges"), ("l012_wall", 3, "scattered")])
def test_fix_mass_flux_over_ranks(name, nranks, kind):
    c = D.case(name)
    got = [None] * nranks
    with VirtualComm(nranks):
        sims, mine, views = rank_sims(c, nranks, kind, uinf=D.UINF, uMax_forced=D.UMAX_FORCED, bFixMassFlux=True)

        def rank(r):
            s = sims[r]
            s.upload("vel", c.vel[mine[r]])
            m = dict(cu.FixMassFlux(s)(D.DT))
            got[r] = (m, s.download("vel"))

        run_ranks(rank, nranks)
        del sims, views
    # each rank's own mean (its sum / volume), then the all-reduce in rank order
    local = [R.fix_mass_flux(c.vel[mine[r]], c.geom[mine[r]], D.UMAX_FORCED, D.NU, D.DT, c.extents, D.UINF)[0]["u_avg_msr"] for r in range(nranks)]
    mean = in_rank_order(local)
    for r in range(nranks):
        want, want_vel = R.fix_mass_flux(c.vel[mine[r]], c.geom[mine[r]], D.UMAX_FORCED, D.NU, D.DT, c.extents, D.UINF, allreduce=lambda _: mean)
        for k in want:
            assert bits(got[r][0][k]) == bits(want[k]), (r, k)
        assert np.array_equal(bits(got[r][1]), bits(want_vel)), r
