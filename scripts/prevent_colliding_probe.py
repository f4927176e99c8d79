"""cup3d_prevent_colliding_obstacles on one device: a uniform 128^3 grid (4096 blocks) and two spheres of radius 1.5, their centres 1.0
apart, each listing the blocks of its own bounding cube, so that the two lists share a few hundred blocks and the bodies overlap in a
lens.  cup3d_create_obstacles runs once and leaves the blocks on the device.  Mean of --calls calls after a first one: device time of
k_collision_sums (cup3d_profile_*; hipEvents on the stream), host wall clock of the whole call (the intersection of the slot lists, the
pair upload, the kernel, 20 doubles per obstacle back, the pair loop) and the bytes that come down.

Measured in the same run, for comparison: the wall clock of uploading the SHARED blocks' chi, udef and sdfLab of both obstacles with
cup3d_sim_upload_block_list -- what a design that stages the blocks per call, as cup3d_penalization does, would pay before its kernel
could start.  sdfLab has no field of its own size: its 1000 doubles per block are stood in for by two scalar block lists (1024).
One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import cup3d_amd as cu  # noqa: E402
from cup3d_amd.capi import ProfileEntry, RunStats, check, lib  # noqa: E402


def profile():
    ents, n = (ProfileEntry * 160)(), C.c_int(0)
    lib().cup3d_profile_read(ents, 160, C.byref(n))
    return {ents[i].name.decode(): (ents[i].launches, ents[i].total_ms) for i in range(n.value)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    cu.device_init(0)
    bc, ext = ("periodic", "wall", "freespace"), 2 * np.pi
    sim = cu.SimulationData(bpdx=2, bpdy=2, bpdz=2, levelMax=4, levelStart=3, extent=ext, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    nb, geom = sim.nblocks, sim.grid.geom
    h = float(geom[0, 0])
    radius = 1.5
    centres = [np.array([np.pi - 0.5, np.pi, np.pi]), np.array([np.pi + 0.5, np.pi + 0.2, np.pi - 0.1])]
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
    sim.shapes = shapes
    cu.CreateObstacles(sim)(0.0)
    motion = [((0.3, 0.05, 0.0), (0.0, 0.02, 0.01)), ((-0.3, 0.0, 0.05), (0.01, 0.0, -0.02))]   # towards each other
    shared = np.intersect1d(shapes[0].slots, shapes[1].slots)
    both = sum(int(((shapes[0].chi[list(shapes[0].slots).index(b)] > 0) & (shapes[1].chi[list(shapes[1].slots).index(b)] > 0)).sum()) for b in shared)
    op = cu.PreventCollidingObstacles(sim)

    def call():
        sim.obstacles = [s.data(v, w) for s, (v, w) in zip(shapes, motion)]   # every call starts from the same motion
        op(0.01)

    out = dict(nblocks=nb, obstacle_blocks=[len(s.slots) for s in shapes], shared_blocks=len(shared), cells_in_both=both, calls=a.calls)
    check(lib().cup3d_profile_enable(1))
    call()   # the first call: module load
    out["resolved"] = bool(sim.obstacles[0].collision_counter > 0)
    check(lib().cup3d_profile_reset())
    check(lib().cup3d_stats_reset())
    wall = 0.0
    for _ in range(a.calls):
        sim.obstacles = [s.data(v, w) for s, (v, w) in zip(shapes, motion)]
        t0 = time.perf_counter()
        op(0.01)
        wall += time.perf_counter() - t0
    prof = profile()
    st = RunStats()
    check(lib().cup3d_stats_read(C.byref(st)))
    check(lib().cup3d_profile_enable(0))
    out["kernel_ms"] = {"collision_sums": prof["collision_sums"][1] / prof["collision_sums"][0]}
    out["call_wall_ms"] = 1e3 * wall / a.calls
    out["bytes_down_per_call"] = st.field_bytes_downloaded / a.calls
    out["field_bytes_up_per_call"] = st.field_bytes_uploaded / a.calls
    out["retained_bytes"] = sum(len(s.slots) for s in shapes) * (4 + 4 * 8 + 1000 * 8 + 512 * 8 + 1536 * 8)
    # what staging the shared blocks per call would upload: chi, udef and sdfLab of both obstacles
    m = len(shared)
    one, three = np.zeros((m, 8, 8, 8)), np.zeros((m, 8, 8, 8, 3))

    def staged():
        for _ in range(2):
            sim.upload_block_list("chi", shared, one)     # chi
            sim.upload_block_list("tmpV", shared, three)  # udef
            sim.upload_block_list("pres", shared, one)    # sdfLab, 1000 doubles per block: two lists of 512
            sim.upload_block_list("lhs", shared, one)

    staged()
    check(lib().cup3d_device_synchronize())
    t0 = time.perf_counter()
    for _ in range(a.calls):
        staged()
    check(lib().cup3d_device_synchronize())
    out["staged_upload_of_shared_blocks"] = dict(wall_ms=1e3 * (time.perf_counter() - t0) / a.calls, bytes=2 * m * (512 + 1536 + 1024) * 8)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
