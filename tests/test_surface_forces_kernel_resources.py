"""What the compiler made of k_surface_forces, the kernel of cup3d_compute_forces (csrc/obstacles_forces.hip), read from the code objects of both
built libraries (no GPU): nothing in scratch, no vector register spilled, no accumulation register, and at most 16 KB of LDS per
workgroup (the 19 x 64 summands of one chunk of points take 9 728 B)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIBS = [os.path.join(ROOT, "cup3d_amd", n) for n in ("libcup3d_hip.so", "libcup3d_hip_testing.so")]


@pytest.mark.parametrize("path", LIBS, ids=["release", "testing"])
def test_surface_forces_kernel_resources(path):
    if not os.path.exists(path):
        import __graft_entry__ as G
        G.build()
    ks = [r for r in KR.kernels(path) if r["kernel"] == "k_surface_forces"]
    assert len(ks) == 1, [r["kernel"] for r in KR.kernels(path) if "surface" in r["kernel"]]
    k = ks[0]
    assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
    assert 19 * 64 * 8 <= k["lds_bytes"] <= 16384, k
    assert k["max_workgroup"] == 64, k   # one wavefront per block: the sums are added in point order by single lanes
