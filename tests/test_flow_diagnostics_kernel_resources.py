"""The kernels of cup3d_compute_dissipation / cup3d_fix_mass_flux (cup3d_amd/csrc/diagnostics.hip) as the built libraries record them
(scripts/kernel_resources.py reads the code objects' own metadata; no GPU): present in both flavours, gfx950 only, no scratch, no spills,
LDS as designed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIBS = ("libcup3d_hip.so", "libcup3d_hip_testing.so")
# LDS by design: k_dissipation = the vel tile 3 x 1040 + the pres tile 1040 + the staged summands 20 x (256 + 1) doubles;
# k_rows_total = one chunk of 1280 doubles; k_mass_flux_sum = one z-plane of 64 doubles; k_mass_flux_add: none
LDS = {"k_dissipation": (4 * 1040 + 20 * 257) * 8, "k_rows_total": 1280 * 8, "k_mass_flux_sum": 64 * 8, "k_mass_flux_add": 0}


@pytest.mark.parametrize("lib", LIBS)
def test_flow_diagnostics_kernels(lib):
    path = os.path.join(ROOT, "cup3d_amd", lib)
    if not os.path.exists(path):
        pytest.fail(f"{lib} is not built")
    rows = {r["kernel"]: r for r in KR.kernels(path)}
    for name, lds in LDS.items():
        assert name in rows, f"{name} is missing from {lib}"
        r = rows[name]
        assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
        assert r["lds_bytes"] == lds, r
        assert r["agpr"] == 0 and r["vgpr"] <= 128, r     # k_dissipation: two workgroups of 256 per CU fit by LDS (2 x 74400 <= 160 KiB) and by registers
    assert 2 * LDS["k_dissipation"] <= 160 * 1024
    assert {t.split("-")[-1] for t, _ in KR.code_objects(path)} == {"gfx950"}
