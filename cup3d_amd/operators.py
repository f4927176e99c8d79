"""Host-side mirror of the reference's Operator / PoissonSolverBase surface for the hot
path, driving the C ABI (include/cup3d_hip.h).  Names, argument meaning and call order
follow slitvinov/CUP3D main.cpp so that tests read like the reference:

    sim = SimulationData(bpdx=.., levelMax=.., BC_x="periodic", nu=.., ...)   # 15330-15387
    pipeline = [AdvectionDiffusion(sim), ExternalForcing(sim), PressureProjection(sim)]  # 15229-15246
    dt = Simulation(sim).calcMaxTimestep(); for op in pipeline: op(dt)                   # 15254-15326

All field data lives on the GPU; host arrays cross the boundary only through
upload()/download() in the reference's block memory layout.  No CPU fallback exists.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import (BC, FIELD_CHI, FIELD_LHS, FIELD_NCOMP, FIELD_PRES, FIELD_TMPV, FIELD_VEL, Cup3dError,
                   PoissonParams, PoissonResult, check, lib)

FIELDS = {"chi": FIELD_CHI, "pres": FIELD_PRES, "vel": FIELD_VEL, "tmpV": FIELD_TMPV, "lhs": FIELD_LHS}


class Grid:
    """Block topology of one rank (host only): GridMPI ownership + m_vInfo order + face
    neighbours + halo plan.  Works without a GPU."""

    def __init__(self, bpd, levelMax, level, maxextent, bc, rank=0, nranks=1, leaves=None):
        """Uniform grid at `level`, or -- with leaves=(levels, Zs) -- the multi-level mesh made of those leaf blocks
        (what MeshAdaptation leaves in m_vInfo; one rank)."""
        self.bpd = np.array(bpd, dtype=np.int32)
        self.bc = np.array([BC[b] if isinstance(b, str) else int(b) for b in bc], dtype=np.int32)
        self.levelMax, self.level, self.maxextent = int(levelMax), int(level), float(maxextent)
        self.rank, self.nranks = int(rank), int(nranks)
        self.multilevel = leaves is not None
        h = C.c_void_p()
        if self.multilevel:
            lv = np.ascontiguousarray(leaves[0], dtype=np.int32)
            zs = np.ascontiguousarray(leaves[1], dtype=np.int64)
            check(lib().cup3d_grid_create_mesh(self.bpd, self.levelMax, self.maxextent, self.bc, len(lv), lv, zs, C.byref(h)))
        else:
            check(lib().cup3d_grid_create_uniform(self.bpd, self.levelMax, self.level, self.maxextent, self.bc,
                                                  self.rank, self.nranks, C.byref(h)))
        self.handle = h
        self.nblocks = lib().cup3d_grid_nblocks(h)
        self.nblocks_global = lib().cup3d_grid_nblocks_global(h)
        self.tables = np.zeros((self.nblocks, 6), dtype=np.int64)
        self.geom = np.zeros((self.nblocks, 4), dtype=np.float64)
        check(lib().cup3d_grid_tables(h, self.tables, self.geom))
        self.index = self.tables[:, 2:5]
        self.h = float(self.geom[0, 0])
        self.ncell = tuple(int(b << self.level) * 8 for b in self.bpd)

    def __del__(self):
        try:
            lib().cup3d_grid_destroy(self.handle)
        except Exception:
            pass

    def valid_states(self, tags):
        """MeshAdaptation::ValidStates (main.cpp:5330-5492) of per-block tags -> the states Adapt will act on."""
        st = np.ascontiguousarray(tags, dtype=np.int8).copy()
        check(lib().cup3d_grid_valid_states(self.handle, st))
        return st

    def adapted_leaves(self, states):
        """(levels, Zs) of the mesh MeshAdaptation::Adapt (5086-5159) produces from valid states."""
        h = C.c_void_p()
        check(lib().cup3d_grid_adapted(self.handle, np.ascontiguousarray(states, dtype=np.int8), C.byref(h)))
        n = lib().cup3d_grid_nblocks(h)
        t, geom = np.zeros((n, 6), dtype=np.int64), np.zeros((n, 4))
        check(lib().cup3d_grid_tables(h, t, geom))
        lib().cup3d_grid_destroy(h)
        return t[:, 0].astype(np.int32), t[:, 1].copy()

    def adapted_owners(self, owner, states, nranks, adapted):
        """Rank of every leaf of `adapted` (a Grid built from self.adapted_leaves(states)) after MeshAdaptation::Adapt and the
        LoadBalancer on `nranks` ranks, given the rank of every leaf of this mesh (cup3d_grid_adapted_owners)."""
        ow = np.ascontiguousarray(owner, dtype=np.int32)
        st = np.ascontiguousarray(states, dtype=np.int8)
        out = np.zeros(adapted.nblocks, dtype=np.int32)
        check(lib().cup3d_grid_adapted_owners(self.handle, ow.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), int(nranks),
                                              adapted.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def rank_view(self, owner, rank, nranks):
        """One rank's view of this multi-level mesh when its leaves are spread over `nranks` ranks as owner[nblocks] says
        (cup3d_grid_rank_view): a RankView with the renumbered tables and the ghost-block / face-flux exchange plans."""
        return RankView(self, owner, rank, nranks)

    def interface(self):
        """Multi-level meshes: (faces[ne,2] = 6*slot+face, kind; fine4[ne,4]; nbr27[nb,27]), see cup3d_grid_interface."""
        ne = lib().cup3d_grid_ninterface_faces(self.handle)
        faces = np.zeros((max(ne, 1), 2), dtype=np.int32)
        fine = np.zeros((max(ne, 1), 4), dtype=np.int32)
        n27 = np.zeros((self.nblocks, 27), dtype=np.int32)
        check(lib().cup3d_grid_interface(self.handle, faces.ctypes.data_as(C.c_void_p), fine.ctypes.data_as(C.c_void_p),
                                         n27.ctypes.data_as(C.c_void_p)))
        return faces[:ne], fine[:ne], n27

    def neighbours(self):
        nbr = np.zeros((self.nblocks, 6), dtype=np.int32)
        check(lib().cup3d_grid_neighbours(self.handle, nbr))
        return nbr

    def halo_plan(self):
        send = np.zeros(self.nranks, dtype=np.int64)
        recv = np.zeros(self.nranks, dtype=np.int64)
        faces = np.zeros(max(1, lib().cup3d_grid_nsend_faces(self.handle)), dtype=np.int32)
        check(lib().cup3d_grid_halo_plan(self.handle, send, recv, faces.ctypes.data_as(C.c_void_p)))
        return send, recv, faces[:lib().cup3d_grid_nsend_faces(self.handle)]

    # global [NZ,NY,NX(,3)] array <-> this rank's blocks in the reference layout
    def to_blocks(self, glob):
        glob = np.asarray(glob, dtype=np.float64)
        out = np.empty((self.nblocks, 8, 8, 8) + glob.shape[3:])
        for s, (i, j, k) in enumerate(self.index):
            out[s] = glob[8 * k:8 * k + 8, 8 * j:8 * j + 8, 8 * i:8 * i + 8]
        return np.ascontiguousarray(out)

    def scatter_to_global(self, blocks, glob):
        for s, (i, j, k) in enumerate(self.index):
            glob[8 * k:8 * k + 8, 8 * j:8 * j + 8, 8 * i:8 * i + 8] = blocks[s]


def uniform_share_mesh(bpd, levelMax, level, maxextent, bc, nranks):
    """What labs_over_ranks needs beside the sims of a uniform grid spread over `nranks` ranks (SimulationData(rank=r, nranks=nranks, ...)):
    the same level as a one-level mesh object, and the owner of each of its leaves -- the contiguous Z-range partition of GridMPI
    (main.cpp:2959-2986), read off the ranks' own Grid objects.  Host only; build it once and pass it to every call.  Returns (mesh, owner)."""
    whole = Grid(bpd, levelMax, level, maxextent, bc)
    mesh = Grid(bpd, levelMax, 0, maxextent, bc, leaves=(whole.tables[:, 0].astype(np.int32), whole.tables[:, 1].copy()))
    rank_of_z = {}
    for r in range(nranks):
        for z in Grid(bpd, levelMax, level, maxextent, bc, r, nranks).tables[:, 1]:
            rank_of_z[int(z)] = r
    owner = np.array([rank_of_z[int(z)] for z in mesh.tables[:, 1]], dtype=np.int32)
    return mesh, owner


class RankView:
    """One rank's view of a multi-level mesh whose leaves are spread over ranks (Grid.rank_view): local blocks, ghost blocks, interface
    faces, neighbour tables in the view's slot numbering, and the two exchange plans (whole ghost blocks before a stencil kernel,
    face-flux arrays after a flux-corrected one).  SimulationData(view=...) runs the operators on it."""

    def __init__(self, mesh, owner, rank, nranks):
        ow = np.ascontiguousarray(owner, dtype=np.int32)
        h = C.c_void_p()
        check(lib().cup3d_grid_rank_view(mesh.handle, ow.ctypes.data_as(C.c_void_p), int(rank), int(nranks), C.byref(h)))
        self.handle, self.rank, self.nranks = h, int(rank), int(nranks)
        self.bpd, self.bc, self.levelMax, self.level, self.maxextent, self.multilevel = mesh.bpd, mesh.bc, mesh.levelMax, mesh.level, mesh.maxextent, True
        self.nblocks = lib().cup3d_grid_nblocks(h)
        self.nblocks_global = lib().cup3d_grid_nblocks_global(h)
        self.tables = np.zeros((self.nblocks, 6), dtype=np.int64)
        self.geom = np.zeros((self.nblocks, 4), dtype=np.float64)
        check(lib().cup3d_grid_tables(h, self.tables, self.geom))
        self.index = self.tables[:, 2:5]
        self.h = mesh.h
        self.ninner = int(lib().cup3d_grid_ninner(h))  # local blocks whose tables lead to no ghost: computed while the ghost blocks travel
        sz = (C.c_long * 6)()
        check(lib().cup3d_grid_view_sizes(h, sz))
        self.nlocal, self.nghost, self.nfaces_local, self.nfaces_ghost, nsb, nsf = (int(v) for v in sz)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self.global_slot = np.zeros(self.nlocal + self.nghost, dtype=np.int32)
        self.global_face = np.zeros(max(self.nfaces_local + self.nfaces_ghost, 1), dtype=np.int32)
        self.send_blocks, self.send_flux_faces = np.zeros(max(nsb, 1), dtype=np.int32), np.zeros(max(nsf, 1), dtype=np.int32)
        counts = [np.zeros(nranks, dtype=np.int64) for _ in range(4)]
        check(lib().cup3d_grid_view_plan(h, p(self.global_slot), p(self.global_face), p(self.send_blocks), p(counts[0]), p(counts[1]),
                                         p(self.send_flux_faces), p(counts[2]), p(counts[3])))
        self.global_face = self.global_face[:self.nfaces_local + self.nfaces_ghost]
        self.send_blocks, self.send_flux_faces = self.send_blocks[:nsb], self.send_flux_faces[:nsf]
        self.send_block_count, self.recv_block_count, self.send_flux_count, self.recv_flux_count = counts
        self.nbr = np.zeros((self.nlocal, 6), dtype=np.int32)
        check(lib().cup3d_grid_neighbours(h, self.nbr.reshape(-1)))
        nf = self.nfaces_local + self.nfaces_ghost
        self.faces, self.fine = np.zeros((max(nf, 1), 2), dtype=np.int32), np.zeros((max(nf, 1), 4), dtype=np.int32)
        self.nbr27 = np.zeros((self.nlocal, 27), dtype=np.int32)
        check(lib().cup3d_grid_interface(h, p(self.faces), p(self.fine), p(self.nbr27)))
        self.faces, self.fine = self.faces[:nf], self.fine[:nf]
        # sub-box form of the ghost-block exchange, per stencil-width class (0: w = 1, 1: w = 3): boxes lo x,y,z / hi x,y,z and cells per rank
        self.ghost_box, self.send_box, self.send_cells, self.recv_cells = [], [], [], []
        for k in (0, 1):
            gb, sb = np.zeros((max(self.nghost, 1), 6), dtype=np.uint8), np.zeros((max(nsb, 1), 6), dtype=np.uint8)
            sc, rc = np.zeros(nranks, dtype=np.int64), np.zeros(nranks, dtype=np.int64)
            check(lib().cup3d_grid_view_boxes(h, k, p(gb), p(sb), p(sc), p(rc)))
            self.ghost_box.append(gb[:self.nghost]); self.send_box.append(sb[:nsb]); self.send_cells.append(sc); self.recv_cells.append(rc)

    def __del__(self):
        try:
            lib().cup3d_grid_destroy(self.handle)
        except Exception:
            pass


class SimulationData:
    """Device-resident counterpart of struct SimulationData (main.cpp:6600-6677): the five
    block grids chi, pres, vel, tmpV, lhs plus the run parameters the hot path reads."""

    def __init__(self, bpdx=1, bpdy=1, bpdz=1, levelMax=1, levelStart=None, extent=1.0, nu=0.0, CFL=0.1,
                 BC_x="freespace", BC_y="freespace", BC_z="freespace", uinf=(0.0, 0.0, 0.0), uMax_forced=0.0,
                 poissonTol=1e-6, poissonTolRel=1e-4, bMeanConstraint=1, poissonSolver="hip_iterative", rampup=100,
                 blockSolver=0, leaves=None, implicitDiffusion=False, diffusionTol=1e-6, diffusionTolRel=1e-4,
                 rank=0, nranks=1, device=None, view=None, diffusionBlockSolver=0, bFixMassFlux=False, freqDiagnostics=100):
        if device is not None or not capi._device_ready:
            capi.device_init(0 if device is None else device)
        self.bpdx, self.bpdy, self.bpdz = bpdx, bpdy, bpdz
        self.levelMax = levelMax
        self.levelStart = levelMax - 1 if levelStart is None else levelStart
        self.maxextent = float(extent)
        # leaves=(levels, Zs): run on that multi-level mesh instead of the uniform grid at levelStart
        # view=RankView: this rank's share of a multi-level mesh spread over several ranks (ghost blocks + exchange plans)
        self.grid = view if view is not None else Grid((bpdx, bpdy, bpdz), levelMax, self.levelStart, self.maxextent, (BC_x, BC_y, BC_z), rank, nranks,
                                                       leaves=leaves)
        # extents / hmin as in _preprocessArguments, main.cpp:15394-15415
        aux = 1 << (levelMax - 1)
        nfe = [bpdx * aux * 8, bpdy * aux * 8, bpdz * aux * 8]
        self.extents = [n / max(nfe) * self.maxextent for n in nfe]
        self.hmin = self.extents[0] / nfe[0]
        self.BCx_flag, self.BCy_flag, self.BCz_flag = BC_x, BC_y, BC_z
        self.nu, self.CFL, self.uinf = float(nu), float(CFL), np.array(uinf, dtype=np.float64)
        self.uMax_forced, self.rampup = float(uMax_forced), int(rampup)
        # -bFixMassFlux / -freqDiagnostics (main.cpp:15359, 15363)
        self.bFixMassFlux, self.freqDiagnostics = bool(bFixMassFlux), int(freqDiagnostics)
        self.PoissonErrorTol, self.PoissonErrorTolRel, self.bMeanConstraint = poissonTol, poissonTolRel, bMeanConstraint
        self.poissonSolver = poissonSolver
        # -implicitDiffusion / -diffusionTol / diffusionTolRel (main.cpp:15368-15370)
        self.implicitDiffusion, self.DiffusionErrorTol, self.DiffusionErrorTolRel = bool(implicitDiffusion), diffusionTol, diffusionTolRel
        self.blockSolver = int(blockSolver)  # 0: block CG as in the reference, 1: direct block solve (fast diagonalisation)
        self.dt, self.dt_old, self.time, self.step, self.step_2nd_start = 0.0, 0.0, 0.0, 0, 2
        self.coefU = np.array([1.5, -2.0, 0.5])
        self.uMax_measured = 0.0
        h = C.c_void_p()
        check(lib().cup3d_sim_create(self.grid.handle, C.byref(h)))
        self.handle = h
        # the block solve of the implicit diffusion's Helmholtz solves -- 0: block CG as in the reference, 1: direct block solve
        self.diffusionBlockSolver = int(diffusionBlockSolver)
        check(lib().cup3d_diffusion_set_block_solver(h, self.diffusionBlockSolver))
        self.pressureSolver = None
        self.last_poisson = None
        self.Rtol, self.Ctol, self.levelMaxVorticity = 1e9, 0.0, levelMax   # -Rtol / -Ctol / -levelMaxVorticity (15340-15342)
        self.obstacles = []            # ObstacleData list (geometry and motion come from the host)
        self.surfaces = []             # ObstacleSurface list: what ComputeForces evaluates
        self.lambda_penal = 1e6        # sim.lambda (-lambda)
        self.bImplicitPenalization = True

    def __del__(self):
        try:
            lib().cup3d_sim_destroy(self.handle)
        except Exception:
            pass

    @property
    def nblocks(self):
        return self.grid.nblocks

    def upload(self, field, blocks):
        fid = FIELDS[field]
        nc = FIELD_NCOMP[fid]
        a = np.ascontiguousarray(blocks, dtype=np.float64)
        want = (self.nblocks, 8, 8, 8, 3) if nc == 3 else (self.nblocks, 8, 8, 8)
        if a.shape != want:
            raise ValueError(f"{field}: expected block array of shape {want}, got {a.shape}")
        check(lib().cup3d_sim_upload(self.handle, fid, a))
        if field == "chi":
            self._chi_uploaded = True   # chi set by hand (tests): PressureProjection lets the library decide which right-hand side to use

    def download(self, field):
        fid = FIELDS[field]
        nc = FIELD_NCOMP[fid]
        out = np.empty((self.nblocks, 8, 8, 8, 3) if nc == 3 else (self.nblocks, 8, 8, 8))
        check(lib().cup3d_sim_download(self.handle, fid, out))
        return out

    def fill(self, field, value):
        check(lib().cup3d_sim_fill(self.handle, FIELDS[field], float(value)))
        if field == "chi":
            self._chi_uploaded = float(value) != 0.0   # chi set (or cleared) by hand, as upload() notes

    def _block_ptrs(self, a):
        return (C.c_void_p * len(a))(*[a[i].ctypes.data for i in range(len(a))])

    def upload_block_list(self, field, slots, blocks):
        """Partial upload: blocks[i] ([8][8][8][(3)], the reference's block layout) -> block slot slots[i]."""
        fid = FIELDS[field]
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        a = np.ascontiguousarray(blocks, dtype=np.float64)
        if a.shape != ((len(sl), 8, 8, 8, 3) if FIELD_NCOMP[fid] == 3 else (len(sl), 8, 8, 8)):
            raise ValueError(f"{field}: block list of shape {a.shape} for {len(sl)} slots")
        check(lib().cup3d_sim_upload_block_list(self.handle, fid, len(sl), sl.ctypes.data_as(C.c_void_p), self._block_ptrs(a)))

    def download_block_list(self, field, slots):
        fid = FIELDS[field]
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        out = np.empty((len(sl), 8, 8, 8, 3) if FIELD_NCOMP[fid] == 3 else (len(sl), 8, 8, 8))
        check(lib().cup3d_sim_download_block_list(self.handle, fid, len(sl), sl.ctypes.data_as(C.c_void_p), self._block_ptrs(out)))
        return out

    def _labs_args(self, field, width, slots):
        fid = FIELDS[field]
        sl = None if slots is None else np.ascontiguousarray(slots, dtype=np.int32)
        n = self.nblocks if sl is None else len(sl)
        L = 8 + 2 * int(width)
        shape = (n, L, L, L, 3) if FIELD_NCOMP[fid] == 3 else (n, L, L, L)
        return fid, sl, n, shape

    def labs(self, field, width, tensorial=False, slots=None, scalar_dir=-1):
        """Ghosted tiles of the listed blocks (all of them, in slot order, when slots is None) for the stencil box
        [-width, width+1), width 1..4, star or tensorial: BlockLab::load + post_load (main.cpp:3623-3787) on the device
        (cup3d_sim_labs).  ndarray [n, L, L, L, nc], L = 8 + 2*width, z, y, x order (nc dropped for scalars, as download does);
        the edge and corner ghosts of a star tile with width <= 2 are NaN.  scalar_dir 0..2: a scalar field's tile as
        BlockLabBC<.., direction> (implicit diffusion).  Only the tiles cross the host boundary, not the field."""
        fid, sl, n, shape = self._labs_args(field, width, slots)
        out = np.empty(shape)
        check(lib().cup3d_sim_labs(self.handle, fid, n, None if sl is None else sl.ctypes.data_as(C.c_void_p), int(width), int(bool(tensorial)),
                                   int(scalar_dir), out.ctypes.data_as(C.c_void_p)))
        return out

    def labs_into(self, ptr, field, width, tensorial=False, slots=None, scalar_dir=-1):
        """The same into device memory at `ptr` (e.g. torch.empty(shape, dtype=torch.float64, device="cuda").data_ptr()), which
        must hold n*L^3*nc doubles: stream-ordered on the library's compute stream, no synchronisation (cup3d_sim_labs_device).
        Returns the shape of the tiles written."""
        fid, sl, n, shape = self._labs_args(field, width, slots)
        check(lib().cup3d_sim_labs_device(self.handle, fid, n, None if sl is None else sl.ctypes.data_as(C.c_void_p), int(width),
                                          int(bool(tensorial)), int(scalar_dir), C.c_void_p(int(ptr))))
        return shape

    def labs_over_ranks(self, field, width, mesh, owner, tensorial=False, slots=None, scalar_dir=-1):
        """labs() when the mesh is spread over ranks (cup3d_sim_labs_over_ranks; BlockLabMPI::load, main.cpp:4648-4658).  mesh / owner:
        the GLOBAL mesh object (a Grid built with leaves=...) and the rank of every leaf; this SimulationData lives on this rank's view of
        it (view=...) or on its share of a uniform grid (rank=, nranks=: see uniform_share_mesh).  slots: local slots; None: every
        local block; an empty list: this rank needs nothing.  COLLECTIVE: every rank calls it with the same field, width and tensorial."""
        fid, sl, n, shape = self._labs_args(field, width, slots)
        ow = np.ascontiguousarray(owner, dtype=np.int32)
        out = np.empty(shape)
        check(lib().cup3d_sim_labs_over_ranks(self.handle, mesh.handle, ow.ctypes.data_as(C.c_void_p), fid, n, None if sl is None else sl.ctypes.data_as(C.c_void_p),
                                              int(width), int(bool(tensorial)), int(scalar_dir), out.ctypes.data_as(C.c_void_p)))
        return out

    def labs_over_ranks_into(self, ptr, field, width, mesh, owner, tensorial=False, slots=None, scalar_dir=-1):
        """The same into device memory at `ptr` (n*L^3*nc doubles; may be 0 for an empty slot list), stream-ordered on the library's
        compute stream behind the exchange (cup3d_sim_labs_over_ranks_device).  Returns the shape of the tiles written."""
        fid, sl, n, shape = self._labs_args(field, width, slots)
        ow = np.ascontiguousarray(owner, dtype=np.int32)
        check(lib().cup3d_sim_labs_over_ranks_device(self.handle, mesh.handle, ow.ctypes.data_as(C.c_void_p), fid, n,
                                                     None if sl is None else sl.ctypes.data_as(C.c_void_p), int(width), int(bool(tensorial)), int(scalar_dir),
                                                     C.c_void_p(int(ptr)) if ptr else None))
        return shape

    def _like(self, **kw):
        """A SimulationData with this one's run parameters on another mesh (leaves=... or view=...), run state carried along."""
        new = SimulationData(bpdx=self.bpdx, bpdy=self.bpdy, bpdz=self.bpdz, levelMax=self.levelMax, levelStart=self.levelStart,
                             extent=self.maxextent, nu=self.nu, CFL=self.CFL, BC_x=self.BCx_flag, BC_y=self.BCy_flag, BC_z=self.BCz_flag,
                             uinf=self.uinf, uMax_forced=self.uMax_forced, poissonTol=self.PoissonErrorTol, poissonTolRel=self.PoissonErrorTolRel,
                             bMeanConstraint=self.bMeanConstraint, poissonSolver=self.poissonSolver, rampup=self.rampup,
                             blockSolver=self.blockSolver, implicitDiffusion=self.implicitDiffusion,
                             diffusionTol=self.DiffusionErrorTol, diffusionTolRel=self.DiffusionErrorTolRel,
                             diffusionBlockSolver=self.diffusionBlockSolver, bFixMassFlux=self.bFixMassFlux,
                             freqDiagnostics=self.freqDiagnostics, **kw)
        new.dt, new.dt_old, new.time, new.step, new.coefU = self.dt, self.dt_old, self.time, self.step, self.coefU.copy()
        new.uMax_measured = self.uMax_measured
        return new

    def adapted(self, states):
        """A new SimulationData on the mesh that MeshAdaptation::Adapt produces from (valid) `states`, with vel and pres
        moved over on the device (refine / compress / copy; chi, lhs and tmpV are adapted without data in the reference
        too, 15188-15190) and the run state carried along.  Simulation::adaptMesh's second half (15184-15193)."""
        lv, zs = self.grid.adapted_leaves(states)
        new = self._like(leaves=(lv, zs))
        for f in ("vel", "pres"):
            check(lib().cup3d_adapt_transfer(self.handle, new.handle, FIELDS[f]))
        return new

    def adapted_over_ranks(self, mesh, owner, states, rank, nranks):
        """The same when the leaves of `mesh` (the GLOBAL mesh object) are spread over ranks as `owner` says and this SimulationData
        lives on rank `rank`'s view of it: MeshAdaptation::Adapt + the LoadBalancer (main.cpp:4660-5022, 5086-5159).  Collective.
        Returns (new SimulationData on this rank's view of the adapted mesh, the adapted global mesh, its owners)."""
        lv, zs = mesh.adapted_leaves(states)
        new_mesh = Grid(mesh.bpd, mesh.levelMax, 0, mesh.maxextent, mesh.bc, leaves=(lv, zs))
        new_owner = mesh.adapted_owners(owner, states, nranks, new_mesh)
        new = self._like(view=new_mesh.rank_view(new_owner, rank, nranks))
        ow = np.ascontiguousarray(owner, dtype=np.int32)
        for f in ("vel", "pres"):
            check(lib().cup3d_adapt_migrate(mesh.handle, ow.ctypes.data_as(C.c_void_p), self.handle, new_mesh.handle,
                                            new_owner.ctypes.data_as(C.c_void_p), new.handle, FIELDS[f]))
        return new, new_mesh, new_owner

    def poisson_params(self):
        p = PoissonParams()
        lib().cup3d_poisson_default_params(C.byref(p))
        p.tol, p.tol_rel, p.mean_constraint = self.PoissonErrorTol, self.PoissonErrorTolRel, self.bMeanConstraint
        p.block_solver = self.blockSolver
        return p

    def checksum(self, field):
        """Wrapping 64-bit sum of the bit patterns of this rank's blocks of `field` (cup3d_sim_checksum): sums over ranks mod 2^64
        are independent of the partition."""
        out = C.c_ulonglong(0)
        check(lib().cup3d_sim_checksum(self.handle, FIELDS[field], C.byref(out)))
        return int(out.value)

    def device_bytes(self):
        return lib().cup3d_sim_device_bytes(self.handle)


class Operator:
    """class Operator, main.cpp:6678-6684."""

    def __init__(self, sim):
        self.sim = sim

    def __call__(self, dt):
        raise NotImplementedError


class AdvectionDiffusion(Operator):
    """AdvectionDiffusion::operator()(dt), main.cpp:9640-9728 (uses sim.dt like KernelAdvectDiffuse, 9465)."""

    def __call__(self, dt):
        s = self.sim
        s.dt = dt
        check(lib().cup3d_advect_diffuse(s.handle, dt, s.nu, s.uinf))


class AdvectionDiffusionImplicit(Operator):
    """AdvectionDiffusionImplicit::operator()(dt), main.cpp:10030-10119 (calls euler(sim.dt)): upwind advection + one Helmholtz
    solve per velocity component (DiffusionSolver, 6719-7147).  `last_diffusion` holds the three solver results."""

    def diffusion_params(self):
        s = self.sim
        p = PoissonParams()
        lib().cup3d_poisson_default_params(C.byref(p))
        p.tol, p.tol_rel = s.DiffusionErrorTol, s.DiffusionErrorTolRel
        return p

    def __call__(self, dt):
        s = self.sim
        s.dt = dt
        res = (PoissonResult * 3)()
        check(lib().cup3d_advect_diffuse_implicit(s.handle, dt, s.nu, s.uinf, C.byref(self.diffusion_params()), res))
        self.last_diffusion = [res[0], res[1], res[2]]
        return self.last_diffusion


class DiffusionSolver:
    """class DiffusionSolver (main.cpp:6719-7147) on the device: right-hand side in sim.lhs, initial guess and result in sim.pres;
    `mydirection` selects the velocity component whose boundary rule the ghosts follow, `dt` the Helmholtz coefficient."""

    def __init__(self, sim):
        self.sim, self.mydirection, self.dt = sim, 0, sim.dt

    def _params(self):
        p = PoissonParams()
        lib().cup3d_poisson_default_params(C.byref(p))
        p.tol, p.tol_rel = self.sim.DiffusionErrorTol, self.sim.DiffusionErrorTolRel
        return p

    def solve(self):
        r = PoissonResult()
        check(lib().cup3d_diffusion_solve(self.sim.handle, self.mydirection, self.dt, self.sim.nu, C.byref(self._params()), C.byref(r)))
        return r

    def lhs(self):
        """_lhs: sim.lhs <- A sim.pres."""
        check(lib().cup3d_diffusion_lhs(self.sim.handle, self.mydirection, self.dt, self.sim.nu))

    def preconditioner(self):
        """_preconditioner on sim.pres in place."""
        check(lib().cup3d_diffusion_preconditioner(self.sim.handle, self.dt, self.sim.nu))


class ComputeVorticity(Operator):
    """ComputeVorticity::operator()(dt), main.cpp:8726-8746: tmpV <- curl(vel) (the input of adaptMesh's tagging)."""

    def __call__(self, dt=0):
        check(lib().cup3d_compute_vorticity(self.sim.handle))


class GradChiOnTmp(Operator):
    """compute<ScalarLab>(GradChiOnTmp(sim), sim.chi), main.cpp:15182 / 8540-8600: the chi-driven edit of the vorticity in tmpV that
    precedes the tagging in adaptMesh (needs sim.Rtol, sim.Ctol, sim.levelMaxVorticity; chi resident)."""

    def __call__(self, dt=0, mesh=None, owner=None):
        """mesh / owner (the global mesh object and the rank of every leaf): the mesh is spread over ranks and this is a collective."""
        s = self.sim
        lmv = int(getattr(s, "levelMaxVorticity", s.levelMax))
        if mesh is None:
            check(lib().cup3d_grad_chi_on_tmp(s.handle, float(s.Rtol), float(s.Ctol), lmv))
        else:
            ow = np.ascontiguousarray(owner, dtype=np.int32)
            check(lib().cup3d_grad_chi_on_tmp_over_ranks(s.handle, mesh.handle, ow.ctypes.data_as(C.c_void_p), float(s.Rtol), float(s.Ctol), lmv))


class ObstacleData:
    """Host-side description of one obstacle for the device operators: the non-null ObstacleBlocks (block slots, chi, udef in the
    reference's layout, main.cpp:7256-7263) and the rigid motion (centre of mass, translation and angular velocity)."""

    def __init__(self, slots, chi, udef, cm, vel, omega, *, forced=(0, 0, 0), block_rotation=(0, 0, 0), vel_imposed=(0, 0, 0), mass=0.0, J=(0, 0, 0, 0, 0, 0)):
        """forced / block_rotation / vel_imposed: Obstacle::bForcedInSimFrame, bBlockRotation and transVel_imposed, read by UpdateObstacles.
        mass / J: Obstacle::mass and J as CreateObstacles left them, read by PreventCollidingObstacles."""
        self.slots = np.ascontiguousarray(slots, dtype=np.int32)
        self.chi = np.ascontiguousarray(chi, dtype=np.float64).reshape(len(self.slots), 8, 8, 8)
        self.udef = np.ascontiguousarray(udef, dtype=np.float64).reshape(len(self.slots), 8, 8, 8, 3)
        self.cm, self.vel, self.omega = (np.array(v, dtype=np.float64) for v in (cm, vel, omega))
        self.force, self.torque = np.zeros(3), np.zeros(3)
        self.forced, self.block_rotation = (tuple(int(bool(v)) for v in f) for f in (forced, block_rotation))
        self.vel_imposed = np.array(vel_imposed, dtype=np.float64)
        # what UpdateObstacles leaves: transVel_computed / angVel_computed, M (29 totals) and the blocks' 29 sums
        self.vel_computed, self.omega_computed, self.totals, self.block_sums = None, None, None, None
        self.mass, self.J = float(mass), np.array(J, dtype=np.float64)
        # u/v/w_collision, ox/oy/oz_collision and collision_counter (7546): written by PreventCollidingObstacles, read by UpdateObstacles;
        # collision_sums: the obstacle's CollisionInfo (20 values) of the last call
        self.collision_vel, self.collision_omega, self.collision_counter, self.collision_sums = np.zeros(3), np.zeros(3), 0.0, None


def _obstacle_array(obstacles):
    from .capi import Obstacle
    arr = (Obstacle * max(1, len(obstacles)))()
    for o, a in zip(obstacles, arr):
        a.nblocks = len(o.slots)
        a.slots, a.chi, a.udef = o.slots.ctypes.data, o.chi.ctypes.data, o.udef.ctypes.data
        for d in range(3):
            a.cm[d], a.vel[d], a.omega[d] = o.cm[d], o.vel[d], o.omega[d]
    return arr


def _body_array(obstacles):
    """cup3d_obstacle_body of every obstacle: the rigid state alone, for the operators that read the blocks CreateObstacles left on the device"""
    arr = (capi.ObstacleBody * max(1, len(obstacles)))()
    for o, a in zip(obstacles, arr):
        for d in range(3):
            a.cm[d], a.vel[d], a.omega[d] = o.cm[d], o.vel[d], o.omega[d]
    return arr


class ObstacleShape:
    """What the host's geometry leaves of one obstacle on this rank (Obstacle::create): the non-null ObstacleBlocks' slots, their signed
    distance sdf [n][10][10][10] (ObstacleBlock::sdfLab, index [z+1][y+1][x+1]) and deformation velocity udef [n][8][8][8][3], plus
    Obstacle::transVel_correction as the previous step left it.  CreateObstacles fills the rest: chi [n][8][8][8], udef_corrected (udef with
    kernelRemoveUdefMomenta applied; `udef` itself stays as the geometry wrote it), cm, mass, J, both corrections (transvel_correction is
    replaced: the next call reads it as oldCorrVel), com_totals [4], udef_totals [13], block_com [n][4], block_momenta [n][13] and the
    surface as a CSR list over the blocks in the order listed: first [n+1], ijk [np][3], dchi [np][3], delta [np]."""

    def __init__(self, slots, sdf, udef, transvel_correction=(0, 0, 0)):
        self.slots = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        n = len(self.slots)
        self.sdf = np.ascontiguousarray(sdf, dtype=np.float64).reshape(n, 10, 10, 10)
        self.udef = np.ascontiguousarray(udef, dtype=np.float64).reshape(n, 8, 8, 8, 3)
        self.transvel_correction = np.array(transvel_correction, dtype=np.float64)
        self.chi = self.udef_corrected = self.cm = self.mass = self.J = self.angvel_correction = None
        self.com_totals = self.udef_totals = self.block_com = self.block_momenta = self.first = self.ijk = self.dchi = self.delta = None

    def data(self, vel, omega, **kw):
        """The ObstacleData of this obstacle for UpdateObstacles / Penalization / PressureProjection: slots, chi, the corrected udef and
        the centre of mass as CreateObstacles left them, the rigid motion and ObstacleData's keywords from the caller."""
        kw.setdefault("mass", self.mass)
        kw.setdefault("J", self.J)
        return ObstacleData(self.slots, self.chi, self.udef_corrected, self.cm, vel, omega, **kw)

    def surface(self, vel, omega):
        """The ObstacleSurface of this obstacle for ComputeForces: the blocks that have surface points, with their corrected udef."""
        keep = np.where(np.diff(self.first) > 0)[0]
        first = np.concatenate([[0], np.cumsum(np.diff(self.first)[keep])]).astype(np.int32)
        return ObstacleSurface(self.slots[keep], first, self.ijk, self.dchi, self.udef_corrected[keep], self.cm, vel, omega)


class CreateObstacles(Operator):
    """CreateObstacles::operator()(dt), main.cpp:13589-13621, from 13596 to 13619 for sim.shapes (ObstacleShape list), after the host
    has run updateUinf / update / create: the resident chi cleared, KernelCharacteristicFunction, kernelComputeGridCoM and the three
    kernel*UdefMomenta (cup3d_create_obstacles).  Fills each ObstacleShape (see there).  Where sim.obstacles lists one ObstacleData per
    shape, their slots, chi, udef and cm are replaced by the new ones -- the rigid motion stays -- and where it is empty it is filled
    with shape.data(0, 0), so that the operators after this one see the new obstacle.  A collective where the grid is spread over ranks."""

    def __call__(self, dt=0):
        s = self.sim
        shapes = getattr(s, "shapes", None)
        if not shapes:
            return
        arr = (capi.ObstacleShape * len(shapes))()
        out = []
        for o, a in zip(shapes, arr):
            n = len(o.slots)
            w = dict(udef=o.udef.copy(), chi=np.zeros((n, 8, 8, 8)), block_com=np.zeros((n, 4)), block_momenta=np.zeros((n, 13)),
                     first=np.zeros(n + 1, dtype=np.int32), ijk=np.zeros((512 * n, 3), dtype=np.int32), dchi=np.zeros((512 * n, 3)), delta=np.zeros(512 * n))
            a.nblocks = n
            a.slots, a.sdf = o.slots.ctypes.data, o.sdf.ctypes.data
            for k, v in w.items():
                setattr(a, k, v.ctypes.data)
            for d in range(3):
                a.transvel_correction[d] = o.transvel_correction[d]
            out.append(w)
        check(lib().cup3d_create_obstacles(s.handle, len(shapes), arr))
        for o, a, w in zip(shapes, arr, out):
            npts = int(w["first"][-1])
            o.chi, o.udef_corrected, o.block_com, o.block_momenta, o.first = w["chi"], w["udef"], w["block_com"], w["block_momenta"], w["first"]
            o.ijk, o.dchi, o.delta = w["ijk"][:npts].copy(), w["dchi"][:npts].copy(), w["delta"][:npts].copy()
            o.transvel_correction, o.angvel_correction = np.array(a.transvel_correction[:]), np.array(a.angvel_correction[:])
            o.cm, o.mass, o.J = np.array(a.cm[:]), float(a.mass), np.array(a.J[:])
            o.com_totals, o.udef_totals = np.array(a.com_totals[:]), np.array(a.udef_totals[:])
        if not s.obstacles:
            s.obstacles = [o.data((0, 0, 0), (0, 0, 0)) for o in shapes]
        elif len(s.obstacles) == len(shapes):
            for d, o in zip(s.obstacles, shapes):
                d.slots, d.chi, d.udef, d.cm = o.slots, o.chi, o.udef_corrected, o.cm.copy()
                d.mass, d.J = o.mass, o.J.copy()
        s.chi_resident = True


class UpdateObstacles(Operator):
    """UpdateObstacles::operator()(dt), main.cpp:13812-13837, for sim.obstacles (ObstacleData list): KernelIntegrateFluidMomenta on the
    resident vel, then kernelFinalizeObstacleVel and Obstacle::computeVelocities without the collision override (cup3d_update_obstacles).
    Leaves in each ObstacleData the new vel / omega (what Penalization then penalises towards), vel_computed / omega_computed, totals
    (M[29]) and block_sums [n][29].  A collective where the grid is spread over ranks.
    With sim.resident_obstacles the blocks, chi and udef are those the last CreateObstacles left on the device
    (cup3d_update_obstacles_resident): one launch for all obstacles, the same bits."""

    def __call__(self, dt):
        s = self.sim
        if not s.obstacles:
            return
        implicit = 1 if s.bImplicitPenalization else 0
        resident = getattr(s, "resident_obstacles", False)
        arr = _body_array(s.obstacles) if resident else _obstacle_array(s.obstacles)
        mot = (capi.ObstacleMotion * len(s.obstacles))()
        sums = [np.zeros((len(o.slots), 29)) for o in s.obstacles]
        for o, m, b in zip(s.obstacles, mot, sums):
            for d in range(3):
                m.forced[d], m.block_rotation[d], m.vel_imposed[d] = o.forced[d], o.block_rotation[d], o.vel_imposed[d]
            m.block_sums = b.ctypes.data
        if resident:
            check(lib().cup3d_update_obstacles_resident(s.handle, dt, s.lambda_penal, implicit, len(s.obstacles), arr, mot))
        else:
            check(lib().cup3d_update_obstacles(s.handle, dt, s.lambda_penal, implicit, len(s.obstacles), arr, mot))
        for o, a, m, b in zip(s.obstacles, arr, mot, sums):
            o.vel, o.omega = np.array(a.vel[:]), np.array(a.omega[:])
            o.vel_computed, o.omega_computed = np.array(m.vel_computed[:]), np.array(m.omega_computed[:])
            o.totals, o.block_sums = np.array(m.totals[:]), b
            if o.collision_counter > 0:   # 13069-13077: the velocities PreventCollidingObstacles stored hold while the counter runs
                o.collision_counter -= dt
                o.vel, o.omega = o.collision_vel.copy(), o.collision_omega.copy()


class PreventCollidingObstacles(Operator):
    """Penalization::preventCollidingObstacles (main.cpp:14009-14324), what Penalization::operator() begins with (14329), for sim.obstacles
    (ObstacleData list, one per shape of the last CreateObstacles, whose blocks the device still holds): the CollisionInfo sums on the
    device, the all-reduces and the elastic collision of every touching pair on the host (cup3d_prevent_colliding_obstacles).  Replaces
    vel / omega of the obstacles of a resolved pair, stores them with collision_counter = 0.01 dt for UpdateObstacles, leaves each
    obstacle's collision_sums and sets sim.bCollision / sim.bCollisionID.  A collective where the grid is spread over ranks."""

    def __call__(self, dt):
        s = self.sim
        s.bCollisionID = []   # 14013
        if not s.obstacles:
            return
        n = len(s.obstacles)
        arr = (capi.ObstacleCollision * n)()
        for o, a in zip(s.obstacles, arr):
            a.mass, a.collision_counter = o.mass, o.collision_counter
            for d in range(3):
                a.cm[d], a.forced[d], a.vel[d], a.omega[d] = o.cm[d], o.forced[d], o.vel[d], o.omega[d]
                a.collision_vel[d], a.collision_omega[d] = o.collision_vel[d], o.collision_omega[d]
            for q in range(6):
                a.J[q] = o.J[q]
        ids = np.zeros(max(1, n * (n - 1)), dtype=np.int32)
        nids, hit = C.c_int(0), C.c_int(0)
        check(lib().cup3d_prevent_colliding_obstacles(s.handle, dt, n, arr, ids.ctypes.data_as(C.c_void_p), C.byref(nids), C.byref(hit)))
        for o, a in zip(s.obstacles, arr):
            o.vel, o.omega = np.array(a.vel[:]), np.array(a.omega[:])
            o.collision_vel, o.collision_omega, o.collision_counter = np.array(a.collision_vel[:]), np.array(a.collision_omega[:]), float(a.collision_counter)
            o.collision_sums = np.array(a.sums[:])
        s.bCollisionID = ids[:nids.value].tolist()
        s.bCollision = bool(getattr(s, "bCollision", False)) or bool(hit.value)   # 14246: set, never cleared


class Penalization(Operator):
    """Penalization::operator()(dt) without the collision model (main.cpp:14326-14341) for sim.obstacles (ObstacleData list):
    KernelPenalization on the resident vel / chi, then the obstacles' force and torque."""

    def __call__(self, dt):
        s = self.sim
        if not s.obstacles:
            return
        implicit = 1 if s.bImplicitPenalization else 0
        if getattr(s, "resident_obstacles", False):   # on the blocks the last CreateObstacles left on the device: one launch, the same bits
            arr = _body_array(s.obstacles)
            check(lib().cup3d_penalization_resident(s.handle, dt, s.lambda_penal, implicit, len(s.obstacles), arr))
        else:
            arr = _obstacle_array(s.obstacles)
            check(lib().cup3d_penalization(s.handle, dt, s.lambda_penal, implicit, len(s.obstacles), arr))
        for o, a in zip(s.obstacles, arr):
            o.force, o.torque = np.array(a.force[:]), np.array(a.torque[:])


class ObstacleSurface:
    """Host-side description of one obstacle's surface for ComputeForces: the ObstacleBlocks that have surface points (block slots, udef in
    the reference's layout), their surface_data as a CSR list -- block i owns points [first[i], first[i+1]), ijk = ix, iy, iz, dchi =
    dchidx, dchidy, dchidz -- the rigid motion, and qoi [n][19], the blocks' nineteen sums (ObstacleBlock::sumQoI order, main.cpp:7289-7307)
    as they stand before the call: eight of them carry on (12283-12293).  Empty lists: this rank holds none of the obstacle's blocks."""

    def __init__(self, slots, first, ijk, dchi, udef, cm, vel, omega, qoi=None):
        self.slots = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        n = len(self.slots)
        self.first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1) if n else np.zeros(1, dtype=np.int32)
        self.ijk = np.ascontiguousarray(ijk, dtype=np.int32).reshape(-1, 3)
        self.dchi = np.ascontiguousarray(dchi, dtype=np.float64).reshape(-1, 3)
        self.udef = np.ascontiguousarray(udef, dtype=np.float64).reshape(n, 8, 8, 8, 3)
        self.cm, self.vel, self.omega = (np.array(v, dtype=np.float64) for v in (cm, vel, omega))
        self.qoi = np.zeros((n, 19)) if qoi is None else np.array(qoi, dtype=np.float64).reshape(n, 19)
        if len(self.first) != n + 1 or len(self.ijk) != len(self.dchi):
            raise ValueError("ObstacleSurface: first needs one entry per block plus one, ijk and dchi one row per point")


class ComputeForces(Operator):
    """ComputeForces::operator()(dt) without Obstacle::computeForces (main.cpp:12496-12503): KernelComputeForces on the device for
    sim.surfaces (ObstacleSurface list) from the resident vel, chi and pres.  Returns [(points [19][npoints], qoi [n][19])] per obstacle
    -- the 19 per-point arrays in the order pX pY pZ P fX fY fZ fxV fyV fzV omegaX omegaY omegaZ vxDef vX vyDef vY vzDef vZ and the
    blocks' sums -- and leaves qoi in the ObstacleSurface, where the next call starts from.
    With sim.resident_obstacles it is ComputeForces::operator() WITH Obstacle::computeForces (13079-13115) for sim.obstacles on the blocks
    the last CreateObstacles left on the device (cup3d_compute_forces_resident): nothing goes up, the blocks' sums stay on the device
    between calls, the return value has the same shape, and each ObstacleData gets surf_force, pres_force, visc_force, surf_torque, drag,
    thrust, Pout, PoutBnd, defPower, defPowerBnd, pLocom, Pthrust, Pdrag, EffPDef, EffPDefBnd, force_totals (the nineteen sums) and the
    returned arrays again as force_points / force_rows."""

    def __call__(self, dt=0, mesh=None, owner=None):
        """mesh / owner (the global mesh object and the rank of every leaf): the mesh is spread over ranks and this is a collective."""
        s = self.sim
        if getattr(s, "resident_obstacles", False):
            return self._resident(mesh, owner)
        surfaces = getattr(s, "surfaces", [])
        arr = (capi.ObstacleSurface * max(1, len(surfaces)))()
        out = []
        for o, a in zip(surfaces, arr):
            points, qoi = np.zeros((19, len(o.ijk))), o.qoi.copy()
            a.nblocks = len(o.slots)
            a.slots, a.first, a.ijk, a.dchi, a.udef = (v.ctypes.data for v in (o.slots, o.first, o.ijk, o.dchi, o.udef))
            a.points, a.qoi = points.ctypes.data, qoi.ctypes.data
            for d in range(3):
                a.cm[d], a.vel[d], a.omega[d] = o.cm[d], o.vel[d], o.omega[d]
            out.append((points, qoi))
        if mesh is None:
            check(lib().cup3d_compute_forces(s.handle, float(s.nu), len(surfaces), arr))
        else:
            ow = np.ascontiguousarray(owner, dtype=np.int32)
            check(lib().cup3d_compute_forces_over_ranks(s.handle, mesh.handle, ow.ctypes.data_as(C.c_void_p), float(s.nu), len(surfaces), arr))
        for o, (_, qoi) in zip(surfaces, out):
            o.qoi = qoi
        return out

    def _resident(self, mesh, owner):
        s = self.sim
        obstacles = s.obstacles
        if not obstacles:
            return []
        arr = (capi.ObstacleForces * len(obstacles))()
        out = []
        for o, shape, a in zip(obstacles, s.shapes, arr):
            per_block = np.diff(shape.first)   # the surface CreateObstacles returned: how many points and rows come back
            points, qoi = np.zeros((19, int(per_block.sum()))), np.zeros((int((per_block > 0).sum()), 19))
            a.points, a.qoi = points.ctypes.data, qoi.ctypes.data
            for d in range(3):
                a.cm[d], a.vel[d], a.omega[d] = o.cm[d], o.vel[d], o.omega[d]
            out.append((points, qoi))
        if mesh is None:
            check(lib().cup3d_compute_forces_resident(s.handle, float(s.nu), len(obstacles), arr))
        else:
            ow = np.ascontiguousarray(owner, dtype=np.int32)
            check(lib().cup3d_compute_forces_resident_over_ranks(s.handle, mesh.handle, ow.ctypes.data_as(C.c_void_p), float(s.nu), len(obstacles), arr))
        for o, a, (points, qoi) in zip(obstacles, arr, out):
            t = np.array(a.totals[:])
            o.force_totals, o.force_points, o.force_rows = t, points, qoi   # what a pipeline, whose return values nobody sees, leaves to read
            o.surf_force, o.pres_force, o.visc_force, o.surf_torque = t[0:3].copy(), t[3:6].copy(), t[6:9].copy(), t[9:12].copy()   # 13089-13100
            o.drag, o.thrust, o.Pout, o.PoutBnd, o.defPower, o.defPowerBnd, o.pLocom = (float(v) for v in t[12:19])                    # 13101-13107
            o.Pthrust, o.Pdrag, o.EffPDef, o.EffPDefBnd = float(a.Pthrust), float(a.Pdrag), float(a.EffPDef), float(a.EffPDefBnd)   # 13108-13114
        return out


class ExternalForcing(Operator):
    """ExternalForcing::operator()(dt), main.cpp:10581-10596."""

    def __call__(self, dt):
        s = self.sim
        d = 1 if s.BCy_flag == "wall" else 2
        check(lib().cup3d_external_forcing(s.handle, s.uMax_forced, s.nu, s.extents[d], dt))


class FixMassFlux(Operator):
    """FixMassFlux::operator()(dt), main.cpp:12218-12248: the measured mean of u + uinf[0] on the device, then the
    parabolic correction of vel.u[0] in place (cup3d_fix_mass_flux).  Leaves the five numbers the reference prints in sim.mass_flux:
    u_avg_msr, u_avg, delta_u, scale, re_tau.  A collective where the grid is spread over ranks."""

    def __call__(self, dt):
        s = self.sim
        out = capi.MassFlux()
        ext, uinf = np.array(s.extents, dtype=np.float64), np.ascontiguousarray(s.uinf, dtype=np.float64)
        check(lib().cup3d_fix_mass_flux(s.handle, s.uMax_forced, s.nu, dt, ext.ctypes.data_as(C.c_void_p),
                                        uinf.ctypes.data_as(C.c_void_p), C.byref(out)))
        s.mass_flux = {k: float(getattr(out, k)) for k in ("u_avg_msr", "u_avg", "delta_u", "scale", "re_tau")}
        return s.mass_flux


class ComputeDissipation(Operator):
    """ComputeDissipation::operator()(dt), main.cpp:10436-10447: every sim.freqDiagnostics steps the 20 flow integrals of KernelDissipation
    (10347-10434) from the resident vel, pres and chi (cup3d_compute_dissipation), all-reduced where the grid is spread over ranks (then a
    collective).  The reference drops them; here they stay in sim.diagnostics = {"step", "time", "qoi": ndarray[20]} (NAMES labels them)
    and are returned.  block_sums=True also keeps this rank's per-block sums [nblocks][20] under "block_sums"."""

    NAMES = ("vorticity_x", "vorticity_y", "vorticity_z", "linear_impulse_x", "linear_impulse_y", "linear_impulse_z",
             "momentum_x", "momentum_y", "momentum_z", "angular_impulse_x", "angular_impulse_y", "angular_impulse_z",
             "angular_momentum_x", "angular_momentum_y", "angular_momentum_z", "pressure_power", "viscous_power", "helicity",
             "kinetic_energy", "vorticity_magnitude")

    def __call__(self, dt=0, block_sums=False):
        s = self.sim
        if s.freqDiagnostics == 0 or s.step % s.freqDiagnostics:   # 10437
            return None
        return self.compute(block_sums)

    def compute(self, block_sums=False):
        """the integrals of the state as it stands, whatever the step"""
        s = self.sim
        qoi = np.zeros(20)
        rows = np.zeros((s.nblocks, 20)) if block_sums else None
        ext = np.array(s.extents, dtype=np.float64)
        check(lib().cup3d_compute_dissipation(s.handle, s.nu, ext.ctypes.data_as(C.c_void_p), qoi.ctypes.data_as(C.c_void_p),
                                              rows.ctypes.data_as(C.c_void_p) if block_sums else None))
        s.diagnostics = {"step": s.step, "time": s.time, "qoi": qoi}
        if block_sums:
            s.diagnostics["block_sums"] = rows
        return qoi


NAMES = ComputeDissipation.NAMES


class ComputeLHS(Operator):
    """ComputeLHS::operator()(dt), main.cpp:9273-9327: lhs <- A(pres)."""

    def __call__(self, dt=0):
        check(lib().cup3d_compute_lhs(self.sim.handle, self.sim.bMeanConstraint))


class PoissonSolverBase:
    """class PoissonSolverBase, main.cpp:8921-8928."""

    def solve(self):
        raise NotImplementedError


class PoissonSolverHIP(PoissonSolverBase):
    """PoissonSolverAMR (main.cpp:9329-9435, solve 14363-14616) on the device: RHS in sim.lhs,
    initial guess and result in sim.pres."""

    def __init__(self, sim):
        self.sim = sim

    def solve(self):
        p, r = self.sim.poisson_params(), PoissonResult()
        check(lib().cup3d_poisson_solve(self.sim.handle, C.byref(p), C.byref(r)))
        self.sim.last_poisson = r
        return r

    def preconditioner(self):
        """_preconditioner on sim.pres in place (getZImplParallel, main.cpp:14704-14745)."""
        check(lib().cup3d_preconditioner(self.sim.handle, self.sim.blockSolver))


def makePoissonSolver(sim):
    """makePoissonSolver, main.cpp:14747-14758.  "iterative" is the reference's CPU solver and
    is not provided here; "cuda_iterative" is the slot the reference reserves for a GPU solver
    (14750) and is accepted as an alias of "hip_iterative"."""
    if sim.poissonSolver in ("hip_iterative", "cuda_iterative"):
        return PoissonSolverHIP(sim)
    if sim.poissonSolver == "iterative":
        raise RuntimeError('Poisson solver: "iterative" is the CPU reference; this library has no CPU path')
    raise ValueError(f'Poisson solver: "{sim.poissonSolver}" unrecognized!')


class PressureProjection(Operator):
    """PressureProjection::operator()(dt), main.cpp:15061-15160."""

    def __init__(self, sim):
        super().__init__(sim)
        self.pressureSolver = makePoissonSolver(sim)  # 15058-15059
        sim.pressureSolver = self.pressureSolver

    def __call__(self, dt):
        s = self.sim
        s.dt = dt
        if s.obstacles:  # tmpV = 0; kernelUpdateTmpV (15066-15082): chi must be resident (sim.upload("chi", ...))
            s.fill("tmpV", 0.0)
            if getattr(s, "resident_obstacles", False):
                check(lib().cup3d_update_tmpv_resident(s.handle, len(s.obstacles)))
            else:
                check(lib().cup3d_update_tmpv(s.handle, len(s.obstacles), _obstacle_array(s.obstacles)))
        # every rank knows whether obstacles exist (the list is replicated, like the reference's obstacle_vector); chi placed by hand
        # without an ObstacleData list (tests) leaves the decision to the library
        by_hand = getattr(s, "_chi_uploaded", False) or getattr(s, "chi_resident", False)
        check(lib().cup3d_sim_set_obstacles(s.handle, 1 if s.obstacles else (-1 if by_hand else 0)))
        p, r = s.poisson_params(), PoissonResult()
        check(lib().cup3d_pressure_project(s.handle, dt, s.step, C.byref(p), C.byref(r)))
        s.last_poisson = r
        return r


class MeshAdaptation:
    """Data-movement half of class MeshAdaptation (main.cpp:5023-5583) for whole-mesh transitions between
    two uniform levels; the tagging decision is returned to the host, which owns the tree."""

    def __init__(self, Rtol, Ctol):
        self.tolerance_for_refinement, self.tolerance_for_compression = float(Rtol), float(Ctol)

    def Tag(self, sim, field="tmpV"):
        """TagLoadedBlock on every block (5566-5582) -> int8 states: 1 Refine, -1 Compress, 0 Leave."""
        st = np.zeros(sim.nblocks, dtype=np.int8)
        check(lib().cup3d_tag_blocks(sim.handle, FIELDS[field], self.tolerance_for_refinement, self.tolerance_for_compression, st))
        return st

    @staticmethod
    def refine(coarse, fine, field):
        """refine_1 + RefineBlocks (5227-5249, 5493-5565) of every block of `coarse` into `fine`."""
        check(lib().cup3d_prolong(coarse.handle, fine.handle, FIELDS[field]))

    @staticmethod
    def compress(fine, coarse, field):
        """compress (5272-5329) of every sibling octet of `fine` into `coarse`."""
        check(lib().cup3d_restrict(fine.handle, coarse.handle, FIELDS[field]))


def findMaxU(sim):
    """findMaxU, main.cpp:8603-8623."""
    out = C.c_double(0.0)
    check(lib().cup3d_max_u(sim.handle, sim.uinf, C.byref(out)))
    return out.value


class Simulation:
    """The time loop of struct Simulation restricted to the hot path (no obstacles, frozen mesh):
    calcMaxTimestep 15254-15305, advance 15306-15326, pipeline order of setupOperators 15229-15246."""

    def __init__(self, sim, obstacle_operators=False, collisions=False, resident_obstacles=False, forces=False, diagnostics=False):
        """obstacle_operators: with sim.obstacles, put UpdateObstacles and Penalization between the forcing and PressureProjection
        (15235-15243) -- the resident obstacle step -- and, where sim.shapes is set (ObstacleShape list), CreateObstacles in front of
        everything.  Off by default: the caller then runs Penalization itself.
        collisions: with obstacle_operators, PreventCollidingObstacles directly in front of Penalization (14329); it needs the blocks
        CreateObstacles leaves on the device, i.e. sim.shapes.
        resident_obstacles: with obstacle_operators, UpdateObstacles, Penalization and PressureProjection's tmpV update read the blocks, chi
        and udef CreateObstacles leaves on the device instead of uploading them per obstacle (sets sim.resident_obstacles); the same
        pipeline and the same bits.  It needs sim.shapes, so that CreateObstacles runs in front of them.
        forces: ComputeForces after PressureProjection, as setupOperators ends (15244), on the retained set: it needs resident_obstacles.
        diagnostics: ComputeDissipation last (15245): every sim.freqDiagnostics steps the 20 flow integrals land in sim.diagnostics.
        With sim.bFixMassFlux and sim.uMax_forced > 0, FixMassFlux takes ExternalForcing's place (15235-15240)."""
        if forces and not resident_obstacles:
            raise ValueError("forces=True needs resident_obstacles=True: ComputeForces in the pipeline reads the blocks CreateObstacles leaves on the device")
        if resident_obstacles and not (obstacle_operators and getattr(sim, "shapes", None)):
            raise ValueError("resident_obstacles=True needs obstacle_operators=True and sim.shapes (an ObstacleShape list): the operators "
                             "read the blocks CreateObstacles leaves on the device")
        self._bind(sim, obstacle_operators, collisions, resident_obstacles, forces, diagnostics)

    def _bind(self, sim, obstacle_operators, collisions, resident_obstacles, forces=False, diagnostics=False):
        """the operators on `sim`: what __init__ does, and adaptMesh / adaptMeshOverRanks again on the adapted SimulationData"""
        self.sim, self.obstacle_operators, self.collisions = sim, bool(obstacle_operators), bool(collisions)
        self.resident_obstacles, self.forces, self.diagnostics = bool(resident_obstacles), bool(forces), bool(diagnostics)
        if self.resident_obstacles or hasattr(sim, "resident_obstacles"):
            sim.resident_obstacles = self.resident_obstacles
        self.pipeline = [AdvectionDiffusionImplicit(sim) if sim.implicitDiffusion else AdvectionDiffusion(sim)]  # 15231-15234
        if sim.uMax_forced > 0:   # 15235-15240
            self.pipeline.append(FixMassFlux(sim) if sim.bFixMassFlux else ExternalForcing(sim))
        shapes = getattr(sim, "shapes", None)   # ObstacleShape list: CreateObstacles comes first, as in setupOperators (15230)
        if self.obstacle_operators and shapes:
            self.pipeline.insert(0, CreateObstacles(sim))
        if self.obstacle_operators and (sim.obstacles or shapes):
            self.pipeline += [UpdateObstacles(sim)] + ([PreventCollidingObstacles(sim)] if self.collisions else []) + [Penalization(sim)]
        self.pipeline.append(PressureProjection(sim))
        if self.forces:
            self.pipeline.append(ComputeForces(sim))   # 15244
        if self.diagnostics:
            self.pipeline.append(ComputeDissipation(sim))   # 15245

    def adaptMesh(self, Rtol, Ctol):
        """Simulation::adaptMesh (15179-15194) without obstacles: vorticity -> tags -> ValidStates -> Adapt.  Replaces
        self.sim (and the operators bound to it) when the mesh changes; returns the valid states."""
        s = self.sim
        ComputeVorticity(s)(0)
        if s.obstacles or getattr(s, "chi_resident", False):   # compute<ScalarLab>(GradChiOnTmp(sim), sim.chi), 15182
            s.Rtol, s.Ctol = Rtol, Ctol
            GradChiOnTmp(s)(0)
        st = s.grid.valid_states(MeshAdaptation(Rtol, Ctol).Tag(s, "tmpV"))
        if (st != 0).any():
            self._bind(s.adapted(st), self.obstacle_operators, self.collisions, self.resident_obstacles, self.forces, self.diagnostics)
        return st

    def adaptMeshOverRanks(self, mesh, owner, rank, nranks, Rtol, Ctol, allgather):
        """Simulation::adaptMesh on a mesh spread over ranks.  mesh / owner: the global mesh object and the rank of every leaf (every
        rank holds them, like the reference's Octree); allgather(int8 array of this rank's tags) -> list of every rank's tags (the
        host's collective: MPI in the shim, torch.distributed or a thread barrier in the tests).  Returns (states, mesh, owner) -- the
        new ones when the mesh changed; self.sim is then this rank's SimulationData on the adapted mesh."""
        s = self.sim
        ComputeVorticity(s)(0)
        if s.obstacles or getattr(s, "chi_resident", False):   # compute<ScalarLab>(GradChiOnTmp(sim), sim.chi), 15182
            s.Rtol, s.Ctol = Rtol, Ctol
            GradChiOnTmp(s)(0, mesh=mesh, owner=owner)
        parts = allgather(MeshAdaptation(Rtol, Ctol).Tag(s, "tmpV"))
        tags = np.zeros(mesh.nblocks, dtype=np.int8)
        ow = np.asarray(owner)
        for r in range(nranks):
            tags[ow == r] = parts[r]          # a rank's blocks appear in the global order inside its view
        st = mesh.valid_states(tags)
        if not (st != 0).any():
            return st, mesh, owner
        new, new_mesh, new_owner = s.adapted_over_ranks(mesh, owner, st, rank, nranks)
        self._bind(new, self.obstacle_operators, self.collisions, self.resident_obstacles, self.forces, self.diagnostics)
        return st, new_mesh, new_owner

    def calcMaxTimestep(self):
        s = self.sim
        s.dt_old = s.dt
        s.uMax_measured = findMaxU(s)
        s.dt = lib().cup3d_calc_max_timestep2(s.hmin, s.uMax_measured, s.nu, s.CFL, s.step, s.rampup, s.dt_old, s.coefU, int(s.implicitDiffusion))
        if s.dt <= 0:
            raise Cup3dError(f"dt <= 0. CFL={s.CFL}, hMin={s.hmin}, sim.uMax_measured={s.uMax_measured}")
        return s.dt

    def advance(self, dt):
        for op in self.pipeline:
            op(dt)
        self.sim.step += 1
        self.sim.time += dt
