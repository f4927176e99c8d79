"""One multigrid V-cycle (block_solver 5, cup3d_amd/csrc/multigrid.hip) restated in plain NumPy on DENSE per-level arrays.  TEST INFRASTRUCTURE.

Written from the prose at the top of multigrid.hip and from mg_vcycle / mg_vcycle_amr, and deliberately NOT from the device's tables: there is
no slot, nbr, parent, leaf or cf table here.  A level l is one (Z, Y, X) array over the whole box at that level's resolution plus two boolean
arrays over its 8^3 blocks -- `leaf[l]` (the block is a leaf of the mesh) and `node[l]` (a leaf or an ancestor of finer leaves).  Neighbours are
the adjacent cells of the dense array, parents are index >> 1, coarse/fine faces are where the adjacent block is no node: everything follows from
cell coordinates and the boundary conditions.  A uniform grid is the mesh whose only leaves are all blocks of the finest level.

Rules (each one is a line of code below; the mutations of MUTATIONS break one rule each, tests/test_multigrid_restatement.py):
  operator      A_l = h_l (sum6 - 6 .), h_l = h_0 / 2^l
  smoother      red-black Gauss-Seidel, red ((x + y + z) even, block-local) first, `sweeps` sweeps per launch inside each 8^3 block with the block's
                ghosts FROZEN at the previous launch's iterate; update (1/6) (((xm + xp) + (ym + yp)) + (zm + zp) - (1/h) b)
  ghosts        behind a non-periodic domain face the block's own face cell, behind a periodic one the wrapped neighbour; behind a face whose
                neighbour exists one level coarser only: 0 on the way down, the coarse cell that contains the ghost cell (final coarse iterate)
                on the way up
  cycle         per level `launches` launches down (the first from zero), residual b - A x with the ghosts of that last iterate, coarse b = SUM of
                the eight children, associated ((a + b) + (c + d)) + ((e + f) + (g + h)) with a, b adjacent in x, c, d one row up in y, e..h one
                layer up in z (k_mg_residual_restrict); b of a leaf is the input; prolongation piecewise constant, added; `launches` launches up
  coarsest      mean of b removed unless the hierarchy has one level; 1 launch x 64 sweeps if the level is one block (one rank), else 16 x 4
  output        x_l on the leaves
generic over the dtype (float64: what the device computes up to FMA contraction and the order of the mean's sum; np.longdouble: the reference).
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

MUTATIONS = ("black_first", "restrict_average", "keep_mean", "prolong_mirrored_octant", "ghosts_refreshed", "one_sweep_fewer",
             "domain_ghost_zero", "coarse_h_not_doubled", "cf_ghosts_stale_on_the_way_down", "cf_ghosts_wrong_half")


def _blocks(a):
    """(Z, Y, X) -> (nbz, nby, nbx, 8, 8, 8)"""
    Z, Y, X = a.shape
    return a.reshape(Z // 8, 8, Y // 8, 8, X // 8, 8).transpose(0, 2, 4, 1, 3, 5)


def _dense(t):
    nz, ny, nx = t.shape[:3]
    return t.transpose(0, 3, 1, 4, 2, 5).reshape(8 * nz, 8 * ny, 8 * nx)


def _cells(m):
    """block mask -> cell mask"""
    return np.repeat(np.repeat(np.repeat(m, 8, 0), 8, 1), 8, 2)


def _finer(a):
    """every cell -> its eight children (piecewise constant)"""
    return np.repeat(np.repeat(np.repeat(a, 2, 0), 2, 1), 2, 2)


def _swap_halves(a, ax):
    """the two 4-cell halves of every 8-cell block exchanged along dense axis `ax`: cell c of a block -> c ^ 4"""
    s = list(a.shape)
    v = a.reshape(s[:ax] + [s[ax] // 8, 2, 4] + s[ax + 1:])
    return np.flip(v, ax + 1).reshape(s)


_Z, _Y, _X = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
RED = ((_X + _Y + _Z) & 1) == 0


class Mesh:
    """bpd (x, y, z), bc (x, y, z) names or codes (1 / "periodic" wraps), h0 = cell size of level 0, leaves [n, 4] = (level, i, j, k)."""

    def __init__(self, bpd, bc, h0, leaves):
        self.bpd, self.h0 = tuple(int(b) for b in bpd), float(h0)
        self.periodic = tuple(b in (1, "periodic") for b in bc)
        self.leaves = np.asarray(leaves, dtype=np.int64).reshape(-1, 4)
        self.nlev = int(self.leaves[:, 0].max()) + 1
        self.leaf = [np.zeros(tuple(b << l for b in self.bpd[::-1]), bool) for l in range(self.nlev)]
        for l, i, j, k in self.leaves:
            self.leaf[l][k, j, i] = True
        self.node = [m.copy() for m in self.leaf]
        for l in range(self.nlev - 2, -1, -1):
            n = self.node[l + 1]
            self.node[l] |= n.reshape(n.shape[0] // 2, 2, n.shape[1] // 2, 2, n.shape[2] // 2, 2).any(axis=(1, 3, 5))
        assert self.node[0].all()

    @classmethod
    def uniform(cls, bpd, level, bc, h):
        n = [b << level for b in bpd]
        ijk = np.stack(np.meshgrid(np.arange(n[0]), np.arange(n[1]), np.arange(n[2]), indexing="ij"), -1).reshape(-1, 3)
        return cls(bpd, bc, h * 2.0 ** level, np.concatenate([np.full((len(ijk), 1), level), ijk], 1))

    def scatter(self, blocks, dtype=np.float64):
        """leaf blocks [n, 8, 8, 8] in the order of `leaves` -> one dense array per level, zero where no leaf is"""
        out = [np.zeros(tuple(8 * s for s in m.shape), dtype) for m in self.leaf]
        for (l, i, j, k), b in zip(self.leaves, blocks):
            out[l][8 * k:8 * k + 8, 8 * j:8 * j + 8, 8 * i:8 * i + 8] = b
        return out

    def gather(self, levels):
        return np.stack([levels[l][8 * k:8 * k + 8, 8 * j:8 * j + 8, 8 * i:8 * i + 8] for l, i, j, k in self.leaves])


class VCycle:
    """z = V(r): per-level dense arrays in, per-level dense arrays out.  depth: number of levels of the hierarchy (default: down to level 0;
    over N ranks the device stops where the partition stops nesting); coarsest: (launches, sweeps) of the coarsest level (default: by the rule
    above); mutation: one of MUTATIONS, for the catalogue that proves an input can tell the cycle from a wrong one."""

    def __init__(self, mesh, dtype=np.float64, launches=2, sweeps=2, depth=None, coarsest=None, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.m, self.dt, self.nu, self.sw, self.mut = mesh, dtype, int(launches), int(sweeps), mutation
        self.lo = 0 if depth is None else mesh.nlev - int(depth)
        assert 0 <= self.lo < mesh.nlev and all(not mesh.leaf[l].any() for l in range(self.lo))
        self.coarsest = coarsest or ((1, 64) if mesh.node[self.lo].size == 1 else (16, 4))
        if mutation == "one_sweep_fewer":
            self.sw, self.coarsest = self.sw - 1, (self.coarsest[0], self.coarsest[1] - 1)
        self.sixth = dtype(1) / dtype(6)

    def h(self, l):
        return self.dt(self.m.h0 * 2.0 ** -(self.m.nlev - 1 if self.mut == "coarse_h_not_doubled" else l))

    def tiles(self, x, l, fill):
        """[nbz, nby, nbx, 10, 10, 10]: every block of x with its six ghost layers.  fill: what stands where level l has no node (None: 0;
        one array; or three arrays, read through the x-, y- and z-faces respectively)."""
        fills = fill if isinstance(fill, tuple) else (fill,)
        node = _cells(self.m.node[l])
        T = None
        for n, f in enumerate(fills):
            G = x if f is None else np.where(node, x, f)
            for ax in range(3):   # dense axis 0, 1, 2 = z, y, x
                pad = [(0, 0)] * 3
                pad[ax] = (1, 1)
                mode = "wrap" if self.m.periodic[2 - ax] else ("constant" if self.mut == "domain_ghost_zero" else "edge")
                G = np.pad(G, pad, mode=mode)
            t = sliding_window_view(G, (10, 10, 10))[::8, ::8, ::8]
            if T is None:
                T = t.copy()
            elif n == 1:
                T[..., :, (0, 9), :] = t[..., :, (0, 9), :]
            else:
                T[..., (0, 9), :, :] = t[..., (0, 9), :, :]
        return T

    @staticmethod
    def sum6(T):
        return ((T[..., 1:9, 1:9, 0:8] + T[..., 1:9, 1:9, 2:10]) + (T[..., 1:9, 0:8, 1:9] + T[..., 1:9, 2:10, 1:9])) + (T[..., 0:8, 1:9, 1:9] + T[..., 2:10, 1:9, 1:9])

    def smooth(self, x, b, l, launches, sweeps, fill, from_zero):
        if self.mut == "ghosts_refreshed":
            launches, sweeps = launches * sweeps, 1
        rb = (self.dt(1) / self.h(l)) * _blocks(b)
        node = _cells(self.m.node[l])
        for n in range(launches):
            T = self.tiles(x, l, None if from_zero and n == 0 else fill)   # the ghosts of this launch: frozen
            I = T[..., 1:9, 1:9, 1:9]
            for _ in range(sweeps):
                for red in ((False, True) if self.mut == "black_first" else (True, False)):
                    I[...] = np.where(RED == red, self.sixth * (self.sum6(T) - rb), I)
            x = np.where(node, _dense(I), 0)
        return x

    def __call__(self, r):
        if self.mut == "cf_ghosts_stale_on_the_way_down":   # the ghost slabs of the previous cycle, not reset
            return self.cycle(r, self.cycle(r, None)[1])[0]
        return self.cycle(r, None)[0]

    def cycle(self, r, stale):
        m, L, lo, dt = self.m, self.m.nlev - 1, self.lo, self.dt
        b, x = [None] * (L + 1), [None] * (L + 1)
        b[L] = np.asarray(r[L], dtype=dt)
        for l in range(L, lo, -1):   # downward leg
            fill = None if stale is None else _finer(stale[l - 1])
            x[l] = self.smooth(np.zeros_like(b[l]), b[l], l, self.nu, self.sw, fill, True)
            res = _blocks(b[l]) - self.h(l) * (self.sum6(self.tiles(x[l], l, fill)) - dt(6) * _blocks(x[l]))
            res = np.where(_cells(m.node[l]), _dense(res), 0)
            s = ((res[0::2, 0::2, 0::2] + res[0::2, 0::2, 1::2]) + (res[0::2, 1::2, 0::2] + res[0::2, 1::2, 1::2])) + \
                ((res[1::2, 0::2, 0::2] + res[1::2, 0::2, 1::2]) + (res[1::2, 1::2, 0::2] + res[1::2, 1::2, 1::2]))
            if self.mut == "restrict_average":
                s = s / dt(8)
            b[l - 1] = s if r[l - 1] is None else np.where(_cells(m.leaf[l - 1]), np.asarray(r[l - 1], dtype=dt), s)
        if L > lo and self.mut != "keep_mean":
            b[lo] = b[lo] - b[lo].sum() / dt(b[lo].size)
        x[lo] = self.smooth(np.zeros_like(b[lo]), b[lo], lo, *self.coarsest, None, True)
        for l in range(lo + 1, L + 1):   # upward leg
            xc = x[l - 1]
            x[l] = np.where(_cells(m.node[l]), x[l] + _finer(_swap_halves(xc, 2) if self.mut == "prolong_mirrored_octant" else xc), 0)
            fill = _finer(xc)
            if self.mut == "cf_ghosts_wrong_half":   # the tangential half of the coarse face: x-faces wrong in y, y-faces in z, z-faces in x
                fill = (_finer(_swap_halves(xc, 1)), _finer(_swap_halves(xc, 0)), _finer(_swap_halves(xc, 2)))
            x[l] = self.smooth(x[l], b[l], l, self.nu, self.sw, fill, False)
        return [None if l < lo else np.where(_cells(m.leaf[l]), x[l], 0) for l in range(L + 1)], x


def vcycle_uniform(r, bpd, level, bc, h, **kw):
    """One cycle on the uniform grid of `level`: r and the result are dense (Z, Y, X) arrays; h is the cell size of that grid."""
    m = Mesh.uniform(bpd, level, bc, h)
    dt = kw.get("dtype", np.float64)
    return VCycle(m, **kw)([None] * level + [np.asarray(r, dtype=dt)])[level]


def vcycle_blocks(mesh, blocks, **kw):
    """One cycle on leaf blocks [n, 8, 8, 8] in the order of mesh.leaves."""
    dt = kw.get("dtype", np.float64)
    return mesh.gather(VCycle(mesh, **kw)(mesh.scatter(blocks, dt)))
