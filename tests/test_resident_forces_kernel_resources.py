"""What the compiler made of the two kernels of cup3d_compute_forces_resident -- k_surface_forces_set (csrc/obstacles_forces.hip) and
k_retained_surface (csrc/obstacles_create.hip) -- read from the code objects of both built libraries (no GPU): one wavefront per surface
row, nothing in scratch, no vector register spilled, no accumulation register.  k_surface_forces_set shares its body with
k_surface_forces and keeps its LDS (the 19 x 64 summands of one chunk of points); k_retained_surface holds sdfLab (8 000 B) and the
block's chi (4 096 B)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIBS = [os.path.join(ROOT, "cup3d_amd", n) for n in ("libcup3d_hip.so", "libcup3d_hip_testing.so")]
NAMES = ("k_surface_forces", "k_surface_forces_set", "k_retained_surface")


@pytest.mark.parametrize("path", LIBS, ids=["release", "testing"])
def test_resident_forces_kernel_resources(path):
    if not os.path.exists(path):
        import __graft_entry__ as G
        G.build()
    found = {r["kernel"]: r for r in KR.kernels(path) if r["kernel"] in NAMES}
    assert sorted(found) == sorted(NAMES), sorted(found)
    for name in ("k_surface_forces_set", "k_retained_surface"):
        k = found[name]
        assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
        assert k["max_workgroup"] == 64, k
    assert found["k_surface_forces_set"]["lds_bytes"] == found["k_surface_forces"]["lds_bytes"], found
    assert 8000 + 4096 <= found["k_retained_surface"]["lds_bytes"] <= 16384, found["k_retained_surface"]
