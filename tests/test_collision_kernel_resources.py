"""What the compiler made of k_collision_sums (csrc/obstacles_collisions.hip), read from the code objects of both built libraries (no GPU): nothing
in scratch, no vector register spilled, no accumulation register, at most 64 vector registers (eight wavefronts per SIMD).  One wavefront
per obstacle; LDS holds the padded rows of one z-plane's summands -- the 14 sums, imag and jmag are the 16 it cannot do without -- plus
the momenta of the cells the two scanning lanes choose from."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIBS = [os.path.join(ROOT, "cup3d_amd", n) for n in ("libcup3d_hip.so", "libcup3d_hip_testing.so")]


@pytest.mark.parametrize("path", LIBS, ids=["release", "testing"])
def test_collision_kernel_resources(path):
    if not os.path.exists(path):
        import __graft_entry__ as G
        G.build()
    found = [r for r in KR.kernels(path) if r["kernel"] == "k_collision_sums"]
    assert len(found) == 1, [r["kernel"] for r in KR.kernels(path)]
    k = found[0]
    assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
    assert 16 * 65 * 8 <= k["lds_bytes"] <= 16384, k
    assert k["max_workgroup"] == 64, k
    assert k["vgpr"] <= 64, k
