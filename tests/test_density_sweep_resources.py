"""CPU-only: the register figures of the density bandwidth sweep's kernel, read from the built library's code objects
(phamers_amd/_codeobj.py): both FULL variants present, nothing spilled, no scratch, and a register count that fits the waves
per SIMD its __launch_bounds__ claims (512 registers per SIMD lane on gfx950, vector and accumulator registers together)."""
import os
import re

import pytest

from tests.helpers import REPO

KERNEL = "phk_kde_sweep_partial_kernel"


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def _claimed_waves_per_simd():
    text = open(os.path.join(REPO, "phamers_amd", "csrc", "density_sweep.hip")).read()
    m = re.search(r"__launch_bounds__\(GT_WAVES \* 64, (\d+)\)\s+void " + KERNEL, text)
    assert m, "the kernel's __launch_bounds__ was not found"
    return int(m.group(1))


def test_sweep_kernel_fits_its_launch_bounds(resources):
    found = {name: r for name, r in resources.items() if KERNEL in name}
    full = [name for name in found if "ILb1E" in name]
    part = [name for name in found if "ILb0E" in name]
    assert len(full) == 2 and len(part) == 2, sorted(found)     # the narrow-tile and the wide-tile shape of each
    waves = _claimed_waves_per_simd()
    assert waves >= 1
    for name, r in found.items():
        assert r["vgpr_spill_count"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["vgpr_count"] <= 512 // waves, (name, r, waves)
    merge = [r for name, r in resources.items() if "phk_kde_sweep_merge_kernel" in name]
    assert merge and all(r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0 for r in merge)
