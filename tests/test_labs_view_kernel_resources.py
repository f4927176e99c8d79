"""What the compiler made of k_labs_view, the ghosted-tile kernel of cup3d_sim_labs_over_ranks (csrc/labs.hip: the phases of k_labs read
through a rank's tensorial view, local blocks from the field array and ghost blocks from the call's pool), read from the code objects
of both built libraries (no GPU): one instantiation per box width, nothing in scratch, no vector register spilled, one component's
fine tile plus the 10^3 coarse shadow tile in LDS and never more than 80 KB, so that two workgroups fit a compute unit.

Scalar registers: the view's source adds three pointers and a count to k_labs' arguments, and all four instantiations run at the
106-SGPR limit.  The compiler parks scalar registers in lanes of a vector register (.sgpr_spill_count; v_writelane / v_readlane, no
memory traffic, scratch stays 0): 6 at w = 1, 6 at w = 2, 2 at w = 3, 2 at w = 4 in this build.  The bounds below are those figures, so
that one more is seen (DESIGN 5b states them too)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIBS = [os.path.join(ROOT, "cup3d_amd", n) for n in ("libcup3d_hip.so", "libcup3d_hip_testing.so")]
SGPR_SPILLS = {1: 6, 2: 6, 3: 2, 4: 2}


@pytest.mark.parametrize("path", LIBS, ids=["release", "testing"])
def test_labs_view_kernel_resources(path):
    if not os.path.exists(path):
        import __graft_entry__ as G
        G.build()
    rows = [r for r in KR.kernels(path) if r["kernel"].startswith("k_labs_view<")]
    assert sorted(r["kernel"] for r in rows) == [f"k_labs_view<i{w}>" for w in (1, 2, 3, 4)]   # each once
    ks = {r["kernel"]: r for r in rows}
    for w in (1, 2, 3, 4):
        k = ks[f"k_labs_view<i{w}>"]
        assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0, k
        assert k["sgpr_spills"] <= SGPR_SPILLS[w], k   # to VGPR lanes, never to memory
        assert ((8 + 2 * w) ** 3 + 1000) * 8 <= k["lds_bytes"] <= 81920, k
        assert k["max_workgroup"] == 256, k
