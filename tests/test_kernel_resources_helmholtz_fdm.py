"""What the compiler made of k_precond_fdm_helm, the direct 8^3 block solve of the implicit diffusion's Helmholtz operator
(cup3d_diffusion_set_block_solver(sim, 1)), read from the code objects inside the built libraries (no GPU).  The kernel is one wavefront
per block with the four transposes in 64 x 9 doubles of LDS, and it is worth having only while it stays free of scratch: it exists to be
bound by its 16 B/cell of traffic, not by anything else."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

RELEASE = os.path.join(ROOT, "cup3d_amd", "libcup3d_hip.so")
TESTING = os.path.join(ROOT, "cup3d_amd", "libcup3d_hip_testing.so")
KERNEL = "k_precond_fdm_helm<i0>"   # a template for its place in the code object alone (csrc/poisson_block.hpp)


@pytest.fixture(scope="module")
def libraries():
    if not (os.path.exists(RELEASE) and os.path.exists(TESTING)):
        import __graft_entry__ as G
        G.build()
    return {path: KR.kernels(path) for path in (RELEASE, TESTING)}


def test_the_kernel_is_in_both_libraries_once(libraries):
    for path, rows in libraries.items():
        assert [r["kernel"] for r in rows].count(KERNEL) == 1, path


def test_registers_lds_and_scratch(libraries):
    for path, rows in libraries.items():
        k = next(r for r in rows if r["kernel"] == KERNEL)
        assert k["scratch_bytes"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, (path, k)
        assert k["lds_bytes"] == 64 * 9 * 8 and k["max_workgroup"] == 64, (path, k)   # kFdmLds: the transposes, pitch 9
        assert k["waves_per_simd"] >= 4, (path, k)


def test_the_release_library_holds_no_debug_variant(libraries):
    names = [r["kernel"] for r in libraries[RELEASE]]
    assert not [n for n in names if n.startswith("k_debug")], names
    # and the Poisson form of the direct solve is still there beside it, with its own table of reciprocals
    assert names.count("k_precond_fdm") == 1
