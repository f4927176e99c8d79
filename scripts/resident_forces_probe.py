"""The staged surface forces (cup3d_compute_forces: the surface list and udef uploaded per obstacle and per call, tiles per obstacle)
against the resident ones (cup3d_compute_forces_resident: the blocks cup3d_create_obstacles left on the device, the surface list rebuilt
there once, tiles per distinct slot, one launch per chunk) on one device and a uniform 128^3 grid (4096 blocks), in the two shapes of
scripts/resident_obstacles_probe.py:

  one_sphere    one sphere of radius 1.5 that lists the 512 blocks of its bounding cube
  eight_bodies  eight spheres of radius 0.7 on a 2 x 2 x 2 lattice, 64 blocks each, no block shared

The staged and the resident call alternate in one process, --calls pairs after a first one; each timed call ends with a device
synchronisation.  Both return the per-point arrays and the blocks' sums; `resident_no_points` is the resident call with points = NULL,
timed in a third slot of every round.  Reported: median, minimum and maximum of the host wall clock of a call, the device time of the
kernel scopes (cup3d_profile_*; hipEvents on the stream, from a separate pass of --calls rounds), the field bytes that come down
(cup3d_run_stats) and the bytes the staged call sends up.  One JSON line on stdout, and in --out if given."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import cup3d_amd as cu  # noqa: E402
from cup3d_amd.capi import ObstacleForces, RunStats, check, lib  # noqa: E402
from resident_obstacles_probe import profile, spheres  # noqa: E402

NU = 0.001
SCOPES = {"staged": ("labs", "surface_forces", "surface_forces_download"),
          "resident": ("labs", "surface_forces_set", "surface_forces_download"),
          "resident_no_points": ("labs", "surface_forces_set", "surface_forces_download")}


def measure(sim, shapes, calls):
    sim.shapes, sim.obstacles = shapes, []
    cu.CreateObstacles(sim)(0.0)
    for o in sim.obstacles:
        o.vel, o.omega = np.array([0.3, 0.05, 0.0]), np.array([0.0, 0.02, 0.01])
    sim.surfaces = [s.surface(o.vel, o.omega) for s, o in zip(shapes, sim.obstacles)]
    n = len(shapes)
    rows, points = sum(len(s.slots) for s in sim.surfaces), sum(len(s.ijk) for s in sim.surfaces)
    staged_op = cu.ComputeForces(sim)
    bare = (ObstacleForces * n)()
    for a, o in zip(bare, sim.obstacles):
        for d in range(3):
            a.cm[d], a.vel[d], a.omega[d] = o.cm[d], o.vel[d], o.omega[d]

    def staged():
        sim.resident_obstacles = False
        staged_op(0.0)

    def resident():
        sim.resident_obstacles = True
        staged_op(0.0)

    def resident_no_points():
        check(lib().cup3d_compute_forces_resident(sim.handle, NU, n, bare))

    variants = dict(staged=staged, resident=resident, resident_no_points=resident_no_points)
    out = dict(obstacles=n, obstacle_blocks=[len(s.slots) for s in shapes], surface_rows=rows, surface_points=points,
               distinct_surface_slots=len(set(int(b) for s in sim.surfaces for b in s.slots)),
               staged_bytes_up_per_call=rows * (4 + 4 * 8 + 4 + 1536 * 8 + 19 * 8) + n * 4 + points * (3 * 4 + 3 * 8))
    L = lib()
    staged()   # the first calls: module load, the tile tables, the scratch
    resident()   # ... and the plans
    resident_no_points()
    check(L.cup3d_device_synchronize())
    wall, down = {k: [] for k in variants}, {}
    st = RunStats()
    for _ in range(calls):
        for key, call in variants.items():
            check(L.cup3d_stats_reset())
            t0 = time.perf_counter()
            call()
            check(L.cup3d_device_synchronize())
            wall[key].append(1e3 * (time.perf_counter() - t0))
            check(L.cup3d_stats_read(C.byref(st)))
            down[key] = st.field_bytes_downloaded
            assert st.field_bytes_uploaded == 0
    for key, call in variants.items():
        check(L.cup3d_profile_enable(1))
        check(L.cup3d_profile_reset())
        for _ in range(calls):
            call()
        check(L.cup3d_device_synchronize())
        prof = profile()
        check(L.cup3d_profile_enable(0))
        scopes = {s: dict(launches_per_call=prof[s][0] / calls, ms_per_call=prof[s][1] / calls) for s in SCOPES[key] if s in prof}
        out[key] = dict(wall_ms_median=statistics.median(wall[key]), wall_ms_min=min(wall[key]), wall_ms_max=max(wall[key]), scopes=scopes,
                        bytes_down_per_call=down[key])
    sim.resident_obstacles = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cu.device_init(0)
    bc, ext = ("periodic", "wall", "freespace"), 2 * np.pi
    sim = cu.SimulationData(bpdx=2, bpdy=2, bpdz=2, levelMax=4, levelStart=3, extent=ext, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], nu=NU)
    rng = np.random.default_rng(0)
    sim.upload("vel", rng.uniform(-1, 1, (sim.nblocks, 8, 8, 8, 3)))
    sim.upload("pres", rng.uniform(-1, 1, (sim.nblocks, 8, 8, 8)))
    geom = sim.grid.geom
    w = 8 * float(geom[0, 0])   # a block's width; 16 blocks per direction
    out = dict(nblocks=sim.nblocks, calls=a.calls)
    out["one_sphere"] = measure(sim, spheres(geom, [np.array([np.pi, np.pi, np.pi])], 1.5), a.calls)
    lattice = [np.array([x, y, z]) * w for x in (6, 10) for y in (6, 10) for z in (6, 10)]
    out["eight_bodies"] = measure(sim, spheres(geom, lattice, 0.7), a.calls)
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
