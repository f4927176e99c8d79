"""The CPU oracle's ghosted tiles (orc_mesh_labs, oracle/cup3d_oracle_amr.c) against the compiled reference's own `lab` output for the
WIDE and TENSORIAL boxes: [-4,5) and [-2,3) tensorial, [-3,4) tensorial, [-4,5) and [-2,3) star.  test_oracle_amr.py pins the oracle up
to [-3,4) star and [-1,2) tensorial; the device tiles of cup3d_sim_labs (tests/test_gpu_labs.py) lean on the oracle for every box
[-w, w+1), w = 1..4, so the wider pin is committed here.  Bit-exact (np.array_equal) on the cells the reference defines
(oracle_lib.lab_mask).  Runs where oracle/_ref/ref_tool was built."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_oracle_amr import LIVE

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EXT = 2 * np.pi
BOXES = [("vel", -4, 5, 1), ("pres", -4, 5, 1), ("vel", -2, 3, 1), ("vel", -3, 4, 1), ("vel", -4, 5, 0), ("pres", -2, 3, 0)]


@pytest.mark.skipif(not O.have_ref_tool(), reason="oracle/_ref/ref_tool not built (no reference tree here)")
@pytest.mark.parametrize("bpd,lmax,bc,passes,rtol", LIVE)
def test_live_wide_and_tensorial_labs(bpd, lmax, bc, passes, rtol):
    sys.path.insert(0, GOLD)
    import make_golden as M
    wd = O.tempfile.mkdtemp(prefix="widelabs_")
    pre = M.amr_mesh_script(wd, bpd, passes, rtol)
    args = O.ref_args(bpd, lmax, 0, EXT, bc)
    _, wd = O.run_ref(pre + ["tables t1.bin"], args, threads=1, workdir=wd)
    t1, _ = O.read_tables(os.path.join(wd, "t1.bin"))
    nb = len(t1)
    assert len(set(t1[:, 0].tolist())) >= (3 if lmax == 4 else 2)
    rng = np.random.default_rng(17)
    vel, pres = rng.uniform(-1, 1, (nb, 8, 8, 8, 3)), rng.uniform(-1, 1, (nb, 8, 8, 8))
    vel.tofile(os.path.join(wd, "velb.bin"))
    pres.tofile(os.path.join(wd, "presb.bin"))
    script = pre + ["loadb vel velb.bin", "loadb pres presb.bin"] + [f"lab {f} {s} {e} {t} lab{i}.bin" for i, (f, s, e, t) in enumerate(BOXES)]
    _, wd = O.run_ref(script, args, threads=1, workdir=wd)
    m = O.OracleMesh(bpd, lmax, EXT, bc, t1[:, 0], t1[:, 1])
    assert np.array_equal(m.tables, t1)
    for i, (f, s, e, t) in enumerate(BOXES):
        field, nc = (vel, 3) if f == "vel" else (pres, 1)
        L = 8 + e - s - 1
        ref = np.fromfile(os.path.join(wd, f"lab{i}.bin")).reshape(nb, L, L, L, nc)
        mask = O.lab_mask(s, e, bool(t))
        assert np.array_equal(m.labs(field, s, e, bool(t))[:, mask], ref[:, mask]), (f, s, e, t)
