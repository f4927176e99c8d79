"""The (mesh, owner map) cases of cup3d_sim_labs_over_ranks, shared by tests/test_gpu_labs_over_ranks.py (the tiles, on the device) and
tests/test_labs_over_ranks_cases.py (no GPU: that the cases are not vacuous).  A helper module, not a test file."""
import os

import numpy as np

import oracle_lib as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXT = 2 * np.pi
NBR_COARSER, NBR_FINER = 0x20000000, -3

MESHES = ("amr_periodic_l01", "amr_mixed_l12", "l012_wall", "l012_box322")
# (kind, ranks, seed): contiguous ranges of the block order on 2 and 3 ranks, scattered owners on 3 and 5
MAPS = (("ranges", 2, 0), ("ranges", 3, 0), ("scattered", 3, 11), ("scattered", 5, 12))
ALL_WIDTHS_MAP = MAPS[2]   # the map on which a mesh also runs w = 2 and 3


def mesh_recipe(name):
    """bpd, levelMax, bc (names), extent, levels, Zs"""
    if name.startswith("amr_"):
        g = np.load(os.path.join(GOLD, name + ".npz"))
        t = g["tables"]
        return (tuple(int(b) for b in g["bpd"]), int(g["level_max"]), tuple(O.BC_NAMES[int(b)] for b in g["bc"]), float(g["extent"]),
                t[:, 0].astype(np.int32), t[:, 1].copy())
    if name == "l012_wall":
        bpd, lmax, bc = (2, 2, 2), 3, ("wall", "freespace", "wall")
        lv, zs = O.build_balanced_mesh(bpd, lmax, bc, [(0, 0, 0, 0), (1, 0, 0, 0)])
    elif name == "l012_box322":   # a non-cubic box, mixed boundary conditions
        bpd, lmax, bc = (3, 2, 2), 3, ("periodic", "wall", "freespace")
        lv, zs = O.build_balanced_mesh(bpd, lmax, bc, [(0, 2, 1, 0), (1, 4, 2, 1), (0, 0, 0, 1)])
    else:
        raise KeyError(name)
    return bpd, lmax, bc, EXT, np.asarray(lv, dtype=np.int32), np.asarray(zs, dtype=np.int64)


def owners(nb, kind, nranks, seed):
    if kind == "ranges":   # contiguous runs of the m_vInfo order, the shape GridMPI / LoadBalancer leave behind
        return (np.arange(nb) * nranks // nb).astype(np.int32)
    rng = np.random.default_rng(seed)   # scattered: random owners from a fixed seed, every rank non-empty
    ow = rng.integers(0, nranks, nb).astype(np.int32)
    ow[rng.permutation(nb)[:nranks]] = np.arange(nranks)
    return ow


def neighbour_reads(tables, nbr27, bpd):
    """Every (block, kind, position, neighbour block) a tile reads: kind 'same' / 'coarser' / 'finer', position 'face' / 'edge' / 'corner'
    (one, two or three axes off centre), from the global nbr27 (mesh.interface()) and the (level, index) of the leaves -- the finer
    leaves behind a position are found by index, as the library's finer tables name them."""
    at = {(int(t[0]), int(t[2]), int(t[3]), int(t[4])): s for s, t in enumerate(tables)}
    out = []
    for b, t in enumerate(tables):
        lev, idx = int(t[0]), (int(t[2]), int(t[3]), int(t[4]))
        for c in range(27):
            if c == 13:
                continue
            code = (c % 3 - 1, (c // 3) % 3 - 1, c // 9 - 1)
            pos = ("face", "edge", "corner")[sum(k != 0 for k in code) - 1]
            v = int(nbr27[b, c])
            if v >= NBR_COARSER:
                out.append((b, "coarser", pos, v - NBR_COARSER))
            elif v >= 0:
                out.append((b, "same", pos, v))
            elif v == NBR_FINER:
                for q in range(8):
                    bits = [(q >> d) & 1 for d in range(3)]
                    if any(code[d] != 0 and bits[d] for d in range(3)):
                        continue
                    n = [int(bpd[d]) << (lev + 1) for d in range(3)]
                    fi = tuple((2 * idx[d] + (-1 if code[d] < 0 else 2 if code[d] > 0 else bits[d])) % n[d] for d in range(3))
                    if (lev + 1,) + fi in at:
                        out.append((b, "finer", pos, at[(lev + 1,) + fi]))
    return out


ALL_CLASSES = {(k, p) for k in ("same", "coarser", "finer") for p in ("face", "edge", "corner")}


def classes_present(reads):
    return {(k, p) for _, k, p, _ in reads}


def classes_crossing(reads, owner):
    return {(k, p) for b, k, p, n in reads if owner[b] != owner[n]}
