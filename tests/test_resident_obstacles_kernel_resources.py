"""What the compiler made of k_fluid_momenta_set, k_penalize_set and k_update_tmpv_set (csrc/obstacles_update.hip, csrc/obstacles_penalization.hip), read from the code objects
of both built libraries (no GPU): nothing in scratch, no vector register spilled, no accumulation register.  k_fluid_momenta_set is
k_fluid_momenta's body on one wavefront per row of the plan, with its padded LDS rows [29][65]; the other two run one 256-thread workgroup
per touched slot."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIBS = [os.path.join(ROOT, "cup3d_amd", n) for n in ("libcup3d_hip.so", "libcup3d_hip_testing.so")]


@pytest.mark.parametrize("path", LIBS, ids=["release", "testing"])
def test_resident_obstacle_kernel_resources(path):
    if not os.path.exists(path):
        import __graft_entry__ as G
        G.build()
    found = {r["kernel"]: r for r in KR.kernels(path)}
    for name, workgroup in (("k_fluid_momenta_set", 64), ("k_penalize_set", 256), ("k_update_tmpv_set", 256)):
        assert name in found, sorted(found)
        k = found[name]
        assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
        assert k["max_workgroup"] == workgroup, k
    assert 29 * 65 * 8 <= found["k_fluid_momenta_set"]["lds_bytes"] <= 16384, found["k_fluid_momenta_set"]
    # the staged kernels share their bodies with these and keep their LDS: the same padded rows, the same four partial sums
    assert found["k_fluid_momenta_set"]["lds_bytes"] == found["k_fluid_momenta"]["lds_bytes"]
    assert found["k_penalize_set"]["lds_bytes"] == found["k_penalize"]["lds_bytes"] == 32 and found["k_update_tmpv_set"]["lds_bytes"] == 0
