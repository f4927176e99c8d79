"""What the compiler made of k_refine and k_grad_chi, the two kernels of mesh adaptation that build their tensorial tile ([-1,2) and
[-2,3)) from the shared lab phases (csrc/labs_setup.hpp, csrc/labs_phases.hpp) and keep it in LDS for their operator, read from the code
objects of both built libraries (no GPU): each exists once, nothing in scratch, no register spilled; k_refine holds ONE component at a
time -- the 10^3 fine tile and the 10^3 coarse shadow tile, the same for the scalar and the vector instantiation; k_grad_chi holds
the 12^3 fine tile, the coarse shadow tile and the scan's one integer; and k_refine<3> needs no more vector registers than the 128 it
took when it held all three components at once."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIBS = [os.path.join(ROOT, "cup3d_amd", n) for n in ("libcup3d_hip.so", "libcup3d_hip_testing.so")]
NAMES = ["k_grad_chi", "k_refine<i1>", "k_refine<i3>"]


@pytest.mark.parametrize("path", LIBS, ids=["release", "testing"])
def test_adapt_kernel_resources(path):
    if not os.path.exists(path):
        import __graft_entry__ as G
        G.build()
    rows = [r for r in KR.kernels(path) if r["kernel"].startswith(("k_refine", "k_grad_chi"))]
    assert sorted(r["kernel"] for r in rows) == NAMES   # each once, and no other instantiation
    ks = {r["kernel"]: r for r in rows}
    for name in NAMES:
        k = ks[name]
        assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 and k["sgpr_spills"] == 0, k
    assert ks["k_refine<i1>"]["lds_bytes"] == ks["k_refine<i3>"]["lds_bytes"] == (10 ** 3 + 10 ** 3) * 8, ks   # one component at a time
    assert ks["k_grad_chi"]["lds_bytes"] <= (12 ** 3 + 10 ** 3) * 8 + 16, ks["k_grad_chi"]
    assert ks["k_refine<i3>"]["vgpr"] <= 128, ks["k_refine<i3>"]
