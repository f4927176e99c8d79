#!/usr/bin/env python3
"""One cup3d_compute_dissipation call (and one cup3d_fix_mass_flux call) on the release library at N^3, all periodic, random fields:
per call, after a warm-up, the device time of each kernel from cup3d_profile_read and the host's wall time; the median over --reps calls.
Beside it the algorithmic traffic (vel 24 + pres 8 + chi 8 = 40 B per cell, ghosts not counted) over the 8 TB/s roof, and the path the
call replaces: the download of vel, pres and chi.

    python scripts/dissipation_probe.py --n 256 512 [--reps 20] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cup3d_amd as cu  # noqa: E402
from cup3d_amd.capi import ProfileEntry, check, lib  # noqa: E402

ROOF = 8e12


def profile():
    ents, n = (ProfileEntry * 200)(), C.c_int(0)
    lib().cup3d_profile_read(ents, 200, C.byref(n))
    return {ents[i].name.decode(): ents[i].total_ms for i in range(min(n.value, 200))}


def measure(n, reps):
    bpd = n // 8
    level = 0
    while bpd % 2 == 0 and bpd > 1:
        bpd //= 2
        level += 1
    sim = cu.SimulationData(bpdx=bpd, bpdy=bpd, bpdz=bpd, levelMax=level + 1, levelStart=level, extent=2 * np.pi, nu=0.01,
                            BC_x="periodic", BC_y="periodic", BC_z="periodic", uMax_forced=1.0, bFixMassFlux=True)
    rng = np.random.default_rng(1)
    nb = sim.nblocks
    sim.upload("vel", rng.uniform(-1, 1, (nb, 8, 8, 8, 3)))
    sim.upload("pres", rng.uniform(-1, 1, (nb, 8, 8, 8)))
    sim.upload("chi", rng.uniform(0, 1, (nb, 8, 8, 8)))
    diss, flux = cu.ComputeDissipation(sim), cu.FixMassFlux(sim)
    sync = lib().cup3d_device_synchronize
    rec = {"n": n, "blocks": nb, "reps": reps, "roof_ms_40B_per_cell": 40.0 * n ** 3 / ROOF * 1e3}
    check(lib().cup3d_profile_enable(1))
    for name, call, kernels in (("compute_dissipation", diss.compute, ("dissipation", "dissipation_total")),
                                ("fix_mass_flux", lambda: flux(0.01), ("mass_flux_sum", "mass_flux_add"))):
        for _ in range(3):
            call()
        sync()
        wall, dev = [], {k: [] for k in kernels}
        for _ in range(reps):
            check(lib().cup3d_profile_reset())
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            p = profile()
            for k in kernels:
                dev[k].append(p.get(k, 0.0))
        rec[name] = {"wall_ms_median": float(np.median(wall)), **{k + "_ms_median": float(np.median(v)) for k, v in dev.items()}}
    check(lib().cup3d_profile_enable(0))
    t0 = time.perf_counter()
    for f in ("vel", "pres", "chi"):
        sim.download(f)
    rec["download_vel_pres_chi_ms"] = (time.perf_counter() - t0) * 1e3
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cu.device_init(0)
    out = []
    for n in a.n:
        rec = measure(n, a.reps)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
