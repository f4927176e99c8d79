"""The staged obstacle operators (cup3d_update_obstacles, cup3d_penalization, cup3d_update_tmpv: chi and udef uploaded per obstacle and
per call) against the resident ones (cup3d_update_obstacles_resident, cup3d_penalization_resident, cup3d_update_tmpv_resident: the blocks
cup3d_create_obstacles left on the device, one launch per operator) on one device and a uniform 128^3 grid (4096 blocks), in two shapes:

  one_sphere    one sphere of radius 1.5 that lists the 512 blocks of its bounding cube -- the shape DESIGN 5b quotes
  eight_bodies  eight spheres of radius 0.7 on a 2 x 2 x 2 lattice, 64 blocks each, no block shared

Per operator the staged and the resident call alternate in one process, --calls pairs after a first one; each timed call ends with a
device synchronisation.  Reported: median, minimum and maximum of the host wall clock of a call, the device time of the kernels
(cup3d_profile_*; hipEvents on the stream, from a separate pass of --calls pairs), the field bytes that come down
(cup3d_run_stats) and the bytes the staged calls send up (slots, geom, chi, udef of every listed block).  Implicit penalisation.
One JSON line on stdout."""
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
from cup3d_amd.capi import ObstacleMotion, ProfileEntry, RunStats, check, lib  # noqa: E402

DT, LAMBDA, IMPLICIT = 0.01, 1e4, 1
SCOPES = {"update_obstacles": ("update_obstacles", "update_obstacles_set"), "penalization": ("penalization", "penalization_set"),
          "update_tmpv": ("update_tmpv", "update_tmpv_set")}


def profile():
    ents, n = (ProfileEntry * 160)(), C.c_int(0)
    lib().cup3d_profile_read(ents, 160, C.byref(n))
    return {ents[i].name.decode(): (ents[i].launches, ents[i].total_ms) for i in range(n.value)}


def spheres(geom, centres, radius):
    h = float(geom[0, 0])
    lo, hi = geom[:, 1:4], geom[:, 1:4] + 8 * h
    i = np.arange(-1, 9) + 0.5
    rng = np.random.default_rng(0)
    shapes = []
    for centre in centres:
        ids = np.where(((hi > centre - radius - h) & (lo < centre + radius + h)).all(axis=1))[0]
        sdf = np.zeros((len(ids), 10, 10, 10))
        for k, b in enumerate(ids):
            o = geom[b, 1:4]
            z, y, x = np.meshgrid(o[2] + h * i, o[1] + h * i, o[0] + h * i, indexing="ij")
            sdf[k] = radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
        shapes.append(cu.ObstacleShape(ids, sdf, 0.1 * rng.uniform(-1, 1, (len(ids), 8, 8, 8, 3))))
    return shapes


def measure(sim, shapes, calls):
    sim.shapes, sim.obstacles = shapes, []
    cu.CreateObstacles(sim)(0.0)
    for o in sim.obstacles:
        o.vel, o.omega = np.array([0.3, 0.05, 0.0]), np.array([0.0, 0.02, 0.01])
    n = len(shapes)
    rows = sum(len(s.slots) for s in shapes)
    staged, body = cu.operators._obstacle_array(sim.obstacles), cu.operators._body_array(sim.obstacles)
    mot = (ObstacleMotion * n)()
    h, L = sim.handle, lib()
    pairs = {
        "update_obstacles": (lambda: check(L.cup3d_update_obstacles(h, DT, LAMBDA, IMPLICIT, n, staged, mot)),
                             lambda: check(L.cup3d_update_obstacles_resident(h, DT, LAMBDA, IMPLICIT, n, body, mot))),
        "penalization": (lambda: check(L.cup3d_penalization(h, DT, LAMBDA, IMPLICIT, n, staged)),
                         lambda: check(L.cup3d_penalization_resident(h, DT, LAMBDA, IMPLICIT, n, body))),
        "update_tmpv": (lambda: check(L.cup3d_update_tmpv(h, n, staged)), lambda: check(L.cup3d_update_tmpv_resident(h, n))),
    }
    out = dict(obstacles=n, obstacle_blocks=[len(s.slots) for s in shapes], rows=rows, distinct_slots=len(set(int(b) for s in shapes for b in s.slots)),
               staged_bytes_up_per_call=rows * (4 + 4 * 8 + 512 * 8 + 1536 * 8))
    bytes0 = sim.device_bytes()
    for name, (a, b) in pairs.items():
        a(), b()   # the first calls: module load, the plan
        check(L.cup3d_device_synchronize())
        wall, down = ([], []), [0.0, 0.0]
        st = RunStats()
        for _ in range(calls):
            for which, call in enumerate((a, b)):
                check(L.cup3d_stats_reset())
                t0 = time.perf_counter()
                call()
                check(L.cup3d_device_synchronize())
                wall[which].append(1e3 * (time.perf_counter() - t0))
                check(L.cup3d_stats_read(C.byref(st)))
                down[which] = st.field_bytes_downloaded
                assert st.field_bytes_uploaded == 0
        check(L.cup3d_profile_enable(1))
        check(L.cup3d_profile_reset())
        for _ in range(calls):
            a(), b()
        prof = profile()
        check(L.cup3d_profile_enable(0))
        res = {}
        for which, key in enumerate(("staged", "resident")):
            launches, ms = prof[SCOPES[name][which]]
            res[key] = dict(wall_ms_median=statistics.median(wall[which]), wall_ms_min=min(wall[which]), wall_ms_max=max(wall[which]),
                            launches_per_call=launches / calls, kernel_ms_per_call=ms / calls, bytes_down_per_call=down[which])
        res["resident_over_staged_median"] = res["resident"]["wall_ms_median"] / res["staged"]["wall_ms_median"]
        out[name] = res
    out["plan_bytes"] = sim.device_bytes() - bytes0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    cu.device_init(0)
    bc, ext = ("periodic", "wall", "freespace"), 2 * np.pi
    sim = cu.SimulationData(bpdx=2, bpdy=2, bpdz=2, levelMax=4, levelStart=3, extent=ext, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    sim.upload("vel", np.random.default_rng(0).uniform(-1, 1, (sim.nblocks, 8, 8, 8, 3)))
    geom = sim.grid.geom
    w = 8 * float(geom[0, 0])   # a block's width; 16 blocks per direction
    out = dict(nblocks=sim.nblocks, calls=a.calls, implicit=IMPLICIT)
    out["one_sphere"] = measure(sim, spheres(geom, [np.array([np.pi, np.pi, np.pi])], 1.5), a.calls)
    lattice = [np.array([x, y, z]) * w for x in (6, 10) for y in (6, 10) for z in (6, 10)]
    out["eight_bodies"] = measure(sim, spheres(geom, lattice, 0.7), a.calls)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
