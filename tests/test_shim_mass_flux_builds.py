"""The C++ shim (cup3d_amd/host/cup3d_hip_operators.h) with FixMassFluxHIP compiles and links into the unmodified reference TU against a
REAL <mpi.h>, and the binary refers to the entry point of the device operator.  A compile-and-link check, modelled on
tests/test_shim_forces_builds.py: the operator itself is pinned bit for bit by tests/test_gpu_fix_mass_flux.py.  Needs the reference sources
and the build container's MPICH: skipped elsewhere, as tests/test_shim_builds.py is (the GPU box only uses prebuilt files)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference/main.cpp"
MPI = "/opt/conda/lib/libmpi.so"


@pytest.mark.skipif(not (os.path.exists(REFERENCE) and os.path.exists(MPI) and os.path.exists(os.path.join(ROOT, "cup3d_amd", "libcup3d_hip.so"))),
                    reason="needs /root/reference, the container's MPICH and the built product library")
def test_shim_with_fix_mass_flux_links(tmp_path):
    out = tmp_path / "ref_tool_hip_mass_flux"
    cmd = ["g++", "-O0", "-std=c++17", "-DCUBISM_ALIGNMENT=64", "-D_BS_=8", "-DDIMENSION=3", "-DNDEBUG", "-fopenmp", "-w", "-DCUP3D_WITH_HIP",
           "-I/opt/conda/include", "-I" + os.path.join(ROOT, "oracle", "refbuild"), f'-DCUP3D_REFERENCE_MAIN="{REFERENCE}"', "-o", str(out),
           os.path.join(ROOT, "oracle", "ref_harness.cpp"), MPI, "-L" + os.path.join(ROOT, "cup3d_amd"), "-lcup3d_hip", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    syms = subprocess.run(["nm", "-D", "--undefined-only", str(out)], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert "cup3d_fix_mass_flux" in syms
    shim = open(os.path.join(ROOT, "cup3d_amd", "host", "cup3d_hip_operators.h")).read()
    assert 'getenv("CUP3D_HIP_MASSFLUX")' in shim and "class FixMassFluxHIP" in shim
