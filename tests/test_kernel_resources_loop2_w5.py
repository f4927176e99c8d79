"""k_loop2_cg_w5<FMA, EV = 6 (kCgProduction), FLHS = true>: the second fused BiCGSTAB loop kernel of uniform grids held to 5 wavefronts per
SIMD (poisson_loops.hpp, loop2_cg5_body), read from the code object inside the release library (no GPU).  The point of the kernel is that it
fits 96 registers WITHOUT scratch -- loop2_cg_body held to the same budget spills 124 B per lane inside its plane loop -- so this pins
exactly that; tests/test_kernel_resources.py (unchanged) pins that the kernels built from loop2_cg_body did not move."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

RELEASE = os.path.join(ROOT, "cup3d_amd", "libcup3d_hip.so")
TESTING = os.path.join(ROOT, "cup3d_amd", "libcup3d_hip_testing.so")
NAME = "k_loop2_cg_w5<b1,i6,b1>"


@pytest.fixture(scope="module")
def libraries():
    if not (os.path.exists(RELEASE) and os.path.exists(TESTING)):
        import __graft_entry__ as G
        G.build()
    return {path: {r["kernel"]: r for r in KR.kernels(path)} for path in (RELEASE, TESTING)}


def test_second_loop_kernel_at_five_wavefronts_has_no_scratch(libraries):
    k = libraries[RELEASE][NAME]
    assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
    assert k["waves_per_simd"] == 5 and k["vgpr"] <= 96, k
    assert k["lds_bytes"] == 7680 and k["max_workgroup"] == 64, k   # the ghosted tile (10 planes of pitch 96 doubles), one wavefront per workgroup


def test_second_loop_kernel_at_five_wavefronts_is_in_the_testing_library(libraries):
    assert NAME in libraries[TESTING], sorted(n for n in libraries[TESTING] if n.startswith("k_loop2_cg"))
