"""cup3d_create_obstacles on the shape DESIGN 5b quotes for the obstacle operators: one device, a uniform 128^3 grid (4096 blocks), one
obstacle -- a sphere of radius 1.5 in the middle of the 2 pi box -- listing the 512 blocks of its bounding cube.  Mean of --calls calls
after a first one: device time of k_characteristic, k_pack_surface, k_udef_momenta and k_remove_udef_momenta (cup3d_profile_*; hipEvents on
the stream), host wall clock of the whole call (staging, kernels, the two block sums, downloads), and the bytes that cross the host
boundary -- and, for comparison, the wall clock of uploading those blocks' chi with cup3d_sim_upload_block_list, which is what a host-side
CreateObstacles costs beside its own arithmetic.  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import cup3d_amd as cu  # noqa: E402
from cup3d_amd.capi import ObstacleShape, ProfileEntry, RunStats, check, lib  # noqa: E402

KERNELS = ("characteristic", "pack_surface", "udef_momenta", "remove_udef_momenta")


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
    centre, radius = np.array([np.pi] * 3), 1.5
    lo, hi = geom[:, 1:4], geom[:, 1:4] + 8 * h
    ids = np.where(((hi > centre - radius - h) & (lo < centre + radius + h)).all(axis=1))[0]
    n = len(ids)
    i = np.arange(-1, 9) + 0.5
    sdf = np.zeros((n, 10, 10, 10))
    for k, b in enumerate(ids):
        o = geom[b, 1:4]
        z, y, x = np.meshgrid(o[2] + h * i, o[1] + h * i, o[0] + h * i, indexing="ij")
        sdf[k] = radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    rng = np.random.default_rng(0)
    udef = 0.1 * rng.uniform(-1, 1, (n, 8, 8, 8, 3))
    w = dict(slots=ids.astype(np.int32), sdf=sdf, udef=udef.copy(), chi=np.zeros((n, 8, 8, 8)), first=np.zeros(n + 1, dtype=np.int32),
             ijk=np.zeros((512 * n, 3), dtype=np.int32), dchi=np.zeros((512 * n, 3)), delta=np.zeros(512 * n))
    arr = (ObstacleShape * 1)()
    arr[0].nblocks = n
    for k, v in w.items():
        setattr(arr[0], k, v.ctypes.data)

    def call():
        w["udef"][...] = udef   # in/out: every call starts from the geometry's udef
        check(lib().cup3d_create_obstacles(sim.handle, 1, arr))

    out = dict(nblocks=nb, obstacle_blocks=n, calls=a.calls)
    check(lib().cup3d_profile_enable(1))
    call()   # the first call: allocations, module load
    check(lib().cup3d_profile_reset())
    check(lib().cup3d_stats_reset())
    t0 = time.perf_counter()
    for _ in range(a.calls):
        call()
    wall = (time.perf_counter() - t0) / a.calls
    prof = profile()
    st = RunStats()
    check(lib().cup3d_stats_read(C.byref(st)))
    check(lib().cup3d_profile_enable(0))
    npoints = int(w["first"][-1])
    out["surface_points"] = npoints
    out["blocks_with_points"] = int((np.diff(w["first"]) > 0).sum())
    out["kernel_ms"] = {k: prof[k][1] / prof[k][0] for k in KERNELS}
    out["call_wall_ms"] = 1e3 * wall
    out["bytes_down_per_call"] = st.field_bytes_downloaded / a.calls
    out["bytes_up_per_call"] = n * (4 + 4 * 8 + 1000 * 8 + 1536 * 8) + (n + 1) * 4   # slots, geometry, sdfLab, udef; first
    chi = w["chi"].copy()
    sim.upload_block_list("chi", ids, chi)
    t0 = time.perf_counter()
    for _ in range(a.calls):
        sim.upload_block_list("chi", ids, chi)
    check(lib().cup3d_device_synchronize())
    out["upload_block_list_chi"] = dict(wall_ms=1e3 * (time.perf_counter() - t0) / a.calls, bytes=n * 512 * 8)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
