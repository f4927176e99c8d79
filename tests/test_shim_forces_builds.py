"""The C++ shim (cup3d_amd/host/cup3d_hip_operators.h) with ComputeForcesHIP compiles and links into the unmodified reference TU against a
REAL <mpi.h>, and the binary refers to both entry points of the device operator (the single-rank one and the collective one).  A link
check of the multi-rank branch only: the single-rank operator is EXECUTED, on the reference's own fish (which run on the GSL stand-ins of
oracle/refbuild/gsl), by tests/test_gpu_dropin.py::test_fish_create_and_forces_through_the_shim.  Needs the reference sources and the build container's MPICH: skipped elsewhere, as
tests/test_shim_builds.py is (the GPU box only uses prebuilt files)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference/main.cpp"
MPI = "/opt/conda/lib/libmpi.so"


@pytest.mark.skipif(not (os.path.exists(REFERENCE) and os.path.exists(MPI) and os.path.exists(os.path.join(ROOT, "cup3d_amd", "libcup3d_hip.so"))),
                    reason="needs /root/reference, the container's MPICH and the built product library")
def test_shim_with_compute_forces_links(tmp_path):
    out = tmp_path / "ref_tool_hip_forces"
    cmd = ["g++", "-O0", "-std=c++17", "-DCUBISM_ALIGNMENT=64", "-D_BS_=8", "-DDIMENSION=3", "-DNDEBUG", "-fopenmp", "-w", "-DCUP3D_WITH_HIP",
           "-I/opt/conda/include", "-I" + os.path.join(ROOT, "oracle", "refbuild"), f'-DCUP3D_REFERENCE_MAIN="{REFERENCE}"', "-o", str(out),
           os.path.join(ROOT, "oracle", "ref_harness.cpp"), MPI, "-L" + os.path.join(ROOT, "cup3d_amd"), "-lcup3d_hip", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    syms = subprocess.run(["nm", "-D", "--undefined-only", str(out)], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    for s in ("cup3d_compute_forces", "cup3d_compute_forces_over_ranks", "cup3d_grid_rank_view"):
        assert s in syms, s
