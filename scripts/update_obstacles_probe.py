"""cup3d_update_obstacles on the shape DESIGN 5b quotes for the obstacle operators: one device, a uniform 128^3 grid (4096 blocks), one
obstacle on 512 blocks.  Mean of --calls calls after a first one: device time of k_fluid_momenta (cup3d_profile_*; hipEvents on the
stream) and host wall clock of the whole call (staging, kernel, download, block sum, 6 x 6 solve), for implicit penalisation off and on --
and, for comparison, the wall clock of fetching the velocity of those 512 blocks with cup3d_sim_download_block_list, which is what a
host-side UpdateObstacles needs instead.  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import cup3d_amd as cu  # noqa: E402
from cup3d_amd.capi import ObstacleMotion, ProfileEntry, RunStats, check, lib  # noqa: E402


def profile():
    ents, n = (ProfileEntry * 160)(), C.c_int(0)
    lib().cup3d_profile_read(ents, 160, C.byref(n))
    return {ents[i].name.decode(): (ents[i].launches, ents[i].total_ms) for i in range(n.value)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=512)
    a = ap.parse_args()
    cu.device_init(0)
    bc, ext = ("periodic", "wall", "freespace"), 2 * np.pi
    sim = cu.SimulationData(bpdx=2, bpdy=2, bpdz=2, levelMax=4, levelStart=3, extent=ext, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2])
    nb = sim.nblocks
    rng = np.random.default_rng(0)
    sim.upload("vel", rng.uniform(-1, 1, (nb, 8, 8, 8, 3)))
    ids = np.sort(rng.choice(nb, size=a.blocks, replace=False))
    ob = cu.ObstacleData(ids, rng.uniform(-0.4, 1.2, (a.blocks, 8, 8, 8)).clip(0.0, 1.0), 0.1 * rng.uniform(-1, 1, (a.blocks, 8, 8, 8, 3)),
                         (3.0, 3.1, 3.2), (0, 0, 0), (0, 0, 0))
    sim.obstacles, sim.lambda_penal = [ob], 1e4
    out = dict(nblocks=nb, obstacle_blocks=a.blocks, calls=a.calls)
    arr = cu.operators._obstacle_array([ob])
    mot = (ObstacleMotion * 1)()
    sums = np.zeros((a.blocks, 29))
    mot[0].block_sums = sums.ctypes.data
    check(lib().cup3d_profile_enable(1))
    for implicit in (0, 1):
        call = lambda: check(lib().cup3d_update_obstacles(sim.handle, 0.01, sim.lambda_penal, implicit, 1, arr, mot))  # noqa: E731
        call()   # the first call: allocations, module load
        check(lib().cup3d_profile_reset())
        check(lib().cup3d_stats_reset())
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call()
        wall = (time.perf_counter() - t0) / a.calls
        launches, ms = profile()["update_obstacles"]
        st = RunStats()
        check(lib().cup3d_stats_read(C.byref(st)))
        out[f"implicit{implicit}"] = dict(kernel_ms=ms / launches, call_wall_ms=1e3 * wall, bytes_down_per_call=st.field_bytes_downloaded / a.calls)
    check(lib().cup3d_profile_enable(0))
    sim.download_block_list("vel", ids)
    t0 = time.perf_counter()
    for _ in range(a.calls):
        sim.download_block_list("vel", ids)
    out["download_block_list_vel"] = dict(wall_ms=1e3 * (time.perf_counter() - t0) / a.calls, bytes=a.blocks * 1536 * 8)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
