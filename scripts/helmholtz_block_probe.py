#!/usr/bin/env python3
"""The two evaluations of the implicit diffusion's block preconditioner on one GPU: the block CG (cup3d_diffusion_set_block_solver 0,
profile scope diffusion_block_cg) against the direct solve (1, diffusion_block_fdm).

    python scripts/helmholtz_block_probe.py block --size 256 [--shifts 0.01,1,6,100] [--reps 10]   one application, per h^2/(nu dt)
    python scripts/helmholtz_block_probe.py step  --size 256 [--shift 1] [--reps 3]                cup3d_advect_diffuse_implicit, both modes

Times come from the library's own hipEvent profile (cup3d_profile_*) after a warm-up application; the step is also timed on the host
clock between device synchronisations.  One JSON line per measurement.  The block CG's cost depends on its input (iterations until the
1e-7 residual), so `block` takes uniform noise, on which it runs its full course, as the solver's right-hand sides make it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cup3d_amd as cu  # noqa: E402
from bench import taylor_green_blocks  # noqa: E402
from cup3d_amd.capi import PoissonParams, PoissonResult, ProfileEntry, check, lib  # noqa: E402

NU = 0.5
SCOPE = {0: "diffusion_block_cg", 1: "diffusion_block_fdm"}


def profile():
    ents = (ProfileEntry * 64)()
    n = C.c_int(0)
    lib().cup3d_profile_read(ents, 64, C.byref(n))
    return {ents[i].name.decode(): (ents[i].launches, ents[i].total_ms) for i in range(n.value)}


def make(size, **kw):
    level = int(round(np.log2(size // 8)))
    return cu.SimulationData(bpdx=1, bpdy=1, bpdz=1, levelMax=level + 1, levelStart=level, extent=2 * np.pi, BC_x="wall", BC_y="wall", BC_z="wall", **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["block", "step"])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--shifts", default="0.01,1,6,100")
    ap.add_argument("--shift", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    cu.device_init(0)
    lib().cup3d_profile_enable(1)
    cells = float(a.size) ** 3
    if a.what == "block":
        sim = make(a.size)
        h = float(sim.grid.h)
        rhs = np.random.default_rng(0).uniform(-1, 1, (sim.nblocks, 8, 8, 8))
        for shift in [float(x) for x in a.shifts.split(",")]:
            dt = h * h / NU / shift
            z = {}
            for mode in (0, 1):
                check(lib().cup3d_diffusion_set_block_solver(sim.handle, mode))
                sim.upload("pres", rhs)
                check(lib().cup3d_diffusion_preconditioner(sim.handle, dt, NU))   # warm-up; its result is compared below
                z[mode] = sim.download("pres")
                lib().cup3d_device_synchronize()
                lib().cup3d_profile_reset()
                for _ in range(a.reps):
                    sim.upload("pres", rhs)
                    check(lib().cup3d_diffusion_preconditioner(sim.handle, dt, NU))
                lib().cup3d_device_synchronize()
                n, ms = profile()[SCOPE[mode]]
                avg = ms / n
                print(json.dumps({"probe": SCOPE[mode], "size": a.size, "h2_over_nu_dt": shift, "launches": n, "avg_ms": round(avg, 4),
                                  "GBps_algorithmic": round(16 * cells / avg / 1e6, 1), "frac_8TBs": round(16 * cells / avg / 1e6 / 8000, 4)}), flush=True)
            print(json.dumps({"probe": "direct_vs_cg", "size": a.size, "h2_over_nu_dt": shift,
                              "max_rel_diff": float(np.abs(z[1] - z[0]).max() / np.abs(z[1]).max())}), flush=True)
    else:
        sim = make(a.size, nu=NU)
        h = float(sim.grid.h)
        dt = h * h / NU / a.shift
        vel0 = taylor_green_blocks(sim.grid, [2 * np.pi] * 3, 1.0)
        p = PoissonParams()
        lib().cup3d_poisson_default_params(C.byref(p))
        uinf = np.zeros(3)
        for mode in (0, 1, 0, 1):
            check(lib().cup3d_diffusion_set_block_solver(sim.handle, mode))
            for rep in range(a.reps + 1):   # the first one warms up (solver vectors, constants)
                sim.upload("vel", vel0)
                sim.fill("pres", 0.0)
                lib().cup3d_device_synchronize()
                lib().cup3d_profile_reset()
                res = (PoissonResult * 3)()
                t0 = time.perf_counter()
                check(lib().cup3d_advect_diffuse_implicit(sim.handle, dt, NU, uinf, C.byref(p), res))
                lib().cup3d_device_synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                if rep == 0:
                    continue
                prof = profile()
                n, ms = prof[SCOPE[mode]]
                print(json.dumps({"probe": "advect_diffuse_implicit", "size": a.size, "h2_over_nu_dt": a.shift, "diffusion_block_solver": mode,
                                  "wall_ms": round(wall, 3), "device_ms": round(sum(v[1] for v in prof.values()), 3),
                                  "block_solve_launches": n, "block_solve_ms": round(ms, 3), "iterations": [res[i].iterations for i in range(3)]}), flush=True)


if __name__ == "__main__":
    main()
