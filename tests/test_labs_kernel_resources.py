"""What the compiler made of k_labs, the ghosted-tile kernel of cup3d_sim_labs (csrc/labs.hip), read from the code objects of both built
libraries (no GPU): nothing in scratch, no vector register spilled, and at most 80 KB of LDS per workgroup, so that two workgroups fit
the 160 KB of a compute unit (the widest tile, 16^3 fine cells plus the 10^3 coarse shadow tile of one component, takes 40 768 B).

Stated deviation from "no spills": the instantiations for w = 1, 2, 3 run at the 106-SGPR limit and the compiler parks TWO scalar
registers in lanes of a vector register (.sgpr_spill_count = 2; v_writelane / v_readlane, no memory traffic, scratch stays 0); w = 4
has none.  The bound below is that figure, so that a third one is seen."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIBS = [os.path.join(ROOT, "cup3d_amd", n) for n in ("libcup3d_hip.so", "libcup3d_hip_testing.so")]


@pytest.mark.parametrize("path", LIBS, ids=["release", "testing"])
def test_labs_kernel_resources(path):
    if not os.path.exists(path):
        import __graft_entry__ as G
        G.build()
    ks = {r["kernel"]: r for r in KR.kernels(path) if r["kernel"].startswith("k_labs<")}
    assert sorted(ks) == [f"k_labs<i{w}>" for w in (1, 2, 3, 4)], sorted(ks)   # one instantiation per box width
    for w in (1, 2, 3, 4):
        k = ks[f"k_labs<i{w}>"]
        assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
        assert k["sgpr_spills"] <= (0 if w == 4 else 2), k   # to VGPR lanes, never to memory (docstring)
        assert ((8 + 2 * w) ** 3 + 1000) * 8 <= k["lds_bytes"] <= 81920, k   # the fine tile and the coarse shadow tile of one component
        assert k["max_workgroup"] == 256, k
