"""CPU-only: the kernels of the likelihood-ranked lookup (phamers_amd/csrc/hosts.hip) are in the built
library, keep nothing in scratch and spill nothing -- the register lists of the selection are indexed statically -- and two
workgroups of the rank kernel (64 KiB of LDS each: the row step's tile) fit a compute unit's 160 KiB."""
import os

import pytest

# kernel -> instantiations: the rank kernel per (guarded / vector loader) x (list of 8 / 16), the merge per list length,
# the pairs kernel per loader
KERNELS = {"phk_host_rank_kernel": 4, "phk_host_merge_kernel": 2, "phk_host_pairs_kernel": 2, "phk_host_column_kernel": 1}
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_host_kernels_are_present_without_scratch_or_spills(resources):
    for kernel, count in KERNELS.items():
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == count, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
            assert 2 * r["lds_bytes"] <= LDS_LIMIT, (name, r)
    assert all(r["lds_bytes"] == 64 * 1024 for name, r in resources.items() if "phk_host_rank_kernel" in name)
