"""The cases of tests/test_gpu_labs_over_ranks.py are not vacuous (no GPU; host entry points of the library only): on every mesh of its
first test the owner maps, taken together, make a tile read EVERY class of neighbour across a rank boundary -- a same-level, a
coarser and a finer neighbour, each behind a face, an edge and a corner.  Derived from the global nbr27 (mesh.interface()) and the owner
arrays the GPU test uses (tests/labs_ranks_cases.py).

Exceptions: none.  Every one of the four meshes has all nine classes (asserted below), and on every mesh the four maps together cross
all nine; so does each scattered map alone.  A map of contiguous ranges may miss some (on amr_periodic_l01 the two ranges, on l012_wall
the three, keep every same-level neighbour pair on one rank); what each map misses is printed."""
import numpy as np
import pytest

import cup3d_amd as cu
import labs_ranks_cases as LC

NO_SUCH_POSITION = {name: set() for name in LC.MESHES}   # classes a mesh does not have at all: none on these meshes


@pytest.mark.parametrize("name", LC.MESHES)
def test_the_owner_maps_cross_every_neighbour_class(name):
    bpd, lmax, bc, ext, lv, zs = LC.mesh_recipe(name)
    mesh = cu.operators.Grid(bpd, lmax, 0, ext, bc, leaves=(lv, zs))
    assert mesh.nblocks <= 110   # "about a hundred blocks": every GPU case takes seconds
    reads = LC.neighbour_reads(mesh.tables, mesh.interface()[2], bpd)
    present = LC.classes_present(reads)
    assert present == LC.ALL_CLASSES - NO_SUCH_POSITION[name], sorted(LC.ALL_CLASSES - present)
    crossed = set()
    for kind, nranks, seed in LC.MAPS:
        ow = LC.owners(mesh.nblocks, kind, nranks, seed)
        assert set(ow.tolist()) == set(range(nranks))   # every rank non-empty
        got = LC.classes_crossing(reads, ow)
        print(name, kind, nranks, "misses", sorted(present - got))
        if kind == "scattered":
            assert got == present, (kind, nranks, sorted(present - got))
        crossed |= got
    assert crossed == present, sorted(present - crossed)


def test_the_uniform_share_helper_names_the_partition():
    """uniform_share_mesh: the one-level mesh holds the blocks of the uniform grid, and owner[] is the Z-range partition the ranks'
    own Grid objects have -- block by block in each rank's order, which is what cup3d_sim_labs_over_ranks checks."""
    bpd, lmax, level, bc = (2, 2, 2), 2, 1, ("periodic", "wall", "freespace")
    for nranks in (2, 3, 8):
        mesh, owner = cu.operators.uniform_share_mesh(bpd, lmax, level, LC.EXT, bc, nranks)
        assert mesh.nblocks == 64 and (mesh.tables[:, 0] == level).all()
        for r in range(nranks):
            g = cu.operators.Grid(bpd, lmax, level, LC.EXT, bc, r, nranks)
            assert np.array_equal(mesh.tables[owner == r][:, :5], g.tables[:, :5])
