"""CPU-only: the three kernels of the paired ROC-area comparison (phamers_amd/csrc/evaluate.hip) are
in the built library, keep nothing in scratch, spill nothing, and hold at most 160 KiB of LDS -- the static part from the code
object (phamers_amd/_codeobj.py) plus, for the bootstrap kernel, the dynamic part its launcher asks for at the row limit."""
import os
import re

import pytest

from tests.helpers import REPO

KERNELS = ("phk_cmp_place_kernel", "phk_cmp_gram_kernel", "phk_cmp_boot_kernel")
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_compare_kernels_are_present_without_scratch_and_within_lds(resources):
    text = open(os.path.join(REPO, "include", "phamers_hip.h")).read()
    max_rows = int(re.search(r"#define PHK_COMPARE_BOOT_MAX_ROWS (\d+)", text).group(1))
    dynamic = {"phk_cmp_boot_kernel": (max_rows + 1) // 2 * 4}     # two 16-bit counters to a word
    for kernel in KERNELS:
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == 1, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
            assert r["lds_bytes"] + dynamic.get(kernel, 0) <= LDS_LIMIT, (name, r)
