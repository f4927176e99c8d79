"""cup3d_sim_labs_over_ranks on the shape DESIGN 5b quotes: one device, 8 thread ranks of the in-process communicator (testing build), a
uniform 128^3 grid (4096 blocks, 512 per rank); every rank asks for 64 of its blocks, vel, [-4,5) tensorial, device variant.  Mean of
--calls calls: device time of the request exchange, the data exchange and k_labs_view (cup3d_profile_*; hipEvents on the stream), host
wall clock of the collective, bytes sent (cup3d_run_stats), and for comparison the bytes of vel + chi of one rank.

The thread ranks share one device and one compute stream: a rank's events bracket the other ranks' work too, so the times are an upper
bound on the plan and kernel cost, and they say nothing about xGMI.  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

os.environ.setdefault("CUP3D_HIP_FLAVOUR", "testing")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cup3d_amd as cu  # noqa: E402
from cup3d_amd.capi import ProfileEntry, RunStats, check, lib  # noqa: E402


def run_ranks(fn, n):
    errs = [None] * n

    def work(r):
        try:
            fn(r)
        except BaseException as e:  # noqa: BLE001
            errs[r] = e

    ts = [threading.Thread(target=work, args=(r,)) for r in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in errs:
        if e is not None:
            raise e


def profile():
    ents, n = (ProfileEntry * 160)(), C.c_int(0)
    lib().cup3d_profile_read(ents, 160, C.byref(n))
    return {ents[i].name.decode(): (ents[i].launches, ents[i].total_ms) for i in range(n.value)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--tiles", type=int, default=64)
    a = ap.parse_args()
    cu.device_init(0)
    bpd, lmax, level, bc, ext, nr = (2, 2, 2), 4, 3, ("periodic", "wall", "freespace"), 2 * np.pi, a.ranks
    mesh, owner = cu.operators.uniform_share_mesh(bpd, lmax, level, ext, bc, nr)
    check(lib().cup3d_debug_virtual_comm(nr))
    sims = [cu.SimulationData(bpdx=2, bpdy=2, bpdz=2, levelMax=lmax, levelStart=level, extent=ext, BC_x=bc[0], BC_y=bc[1], BC_z=bc[2], rank=r, nranks=nr)
            for r in range(nr)]
    rng = np.random.default_rng(0)
    for s in sims:
        s.upload("vel", rng.uniform(-1, 1, (s.nblocks, 8, 8, 8, 3)))
    out = [torch.empty((a.tiles, 16, 16, 16, 3), dtype=torch.float64, device="cuda") for _ in range(nr)]
    torch.cuda.synchronize()
    res = {"what": "cup3d_sim_labs_over_ranks_device, uniform 128^3 (4096 blocks) on %d thread ranks of one device, %d tiles per rank, vel, [-4,5) tensorial" % (nr, a.tiles),
           "calls": a.calls}
    st = RunStats()
    for label, slots in (("compact", [np.arange(a.tiles, dtype=np.int32) for s in sims]),
                         ("spread", [(np.arange(a.tiles) * (s.nblocks // a.tiles)).astype(np.int32) for s in sims])):
        def call(r):
            sims[r].labs_over_ranks_into(out[r].data_ptr(), "vel", 4, mesh, owner, tensorial=True, slots=slots[r])

        run_ranks(call, nr)   # builds and caches the view; first allocations
        check(lib().cup3d_device_synchronize())
        check(lib().cup3d_profile_enable(1))
        check(lib().cup3d_profile_reset())
        check(lib().cup3d_stats_reset())
        t0 = time.perf_counter()
        for _ in range(a.calls):
            run_ranks(call, nr)
        check(lib().cup3d_device_synchronize())
        wall = time.perf_counter() - t0
        p = profile()
        check(lib().cup3d_profile_enable(0))
        check(lib().cup3d_stats_read(C.byref(st)))
        ms = lambda k: round(p[k][1] / max(1, p[k][0]), 4) if k in p else None  # noqa: E731
        res[label] = {"slots": "the first %d blocks of each rank" % a.tiles if label == "compact" else "every %dth block of each rank" % (sims[0].nblocks // a.tiles),
                      "request_exchange_ms_per_rank_call": ms("labs_request"), "data_exchange_ms_per_rank_call": ms("labs_data"),
                      "k_labs_view_ms_per_rank_call": ms("labs_view"), "host_wall_ms_per_collective_call": round(wall / a.calls * 1e3, 3),
                      "bytes_sent_per_call_all_ranks": st.halo_bytes_sent / a.calls, "bytes_sent_per_call_per_rank": st.halo_bytes_sent / a.calls / nr,
                      "tile_bytes_per_rank": a.tiles * 16 ** 3 * 3 * 8}
    res["vel_plus_chi_bytes_of_one_rank"] = sims[0].nblocks * 4 * 512 * 8
    del sims
    lib().cup3d_device_synchronize()
    lib().cup3d_debug_virtual_comm(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
