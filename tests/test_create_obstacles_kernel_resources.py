"""What the compiler made of the three kernels of cup3d_create_obstacles (csrc/obstacles_create.hip) and of the copy kernel between them, read
from the code objects of both built libraries (no GPU): nothing in scratch, no vector register spilled, no accumulation register.
k_characteristic holds sdfLab (8 000 B), the block's chi (4 096 B) and four padded rows of summands (2 080 B) in LDS; k_udef_momenta the
13 x 65 summands of one z-plane (6 760 B).  Both run one wavefront per block: the sums are added in cell order by single lanes."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIBS = [os.path.join(ROOT, "cup3d_amd", n) for n in ("libcup3d_hip.so", "libcup3d_hip_testing.so")]
# kernel -> (LDS bytes at least, at most, workgroup size)
WANT = {"k_characteristic": (8000 + 4096 + 4 * 64 * 8, 16384, 64), "k_udef_momenta": (13 * 64 * 8, 8192, 64), "k_remove_udef_momenta": (0, 0, 256),
        "k_pack_surface": (0, 0, 64)}


@pytest.mark.parametrize("path", LIBS, ids=["release", "testing"])
def test_create_obstacles_kernel_resources(path):
    if not os.path.exists(path):
        import __graft_entry__ as G
        G.build()
    found = {r["kernel"]: r for r in KR.kernels(path) if r["kernel"] in WANT}
    assert sorted(found) == sorted(WANT), sorted(found)
    for name, (lo, hi, wg) in WANT.items():
        k = found[name]
        assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
        assert lo <= k["lds_bytes"] <= hi, k
        assert k["max_workgroup"] == wg, k
        assert k["vgpr"] <= 64, k   # eight wavefronts per SIMD
