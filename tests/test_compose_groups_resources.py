"""CPU-only: the kernels of the grouped chain (phamers_amd/csrc/chain.hip) are in the built library --
the per-record kernels once per padded state count (2, 4, 8), the two matrix-pipe kernels once per loader variant --, keep
nothing in scratch and spill nothing, the per-record ones use no LDS; no new kernel counts as one of the kernels the older
resource tests count by substring; the three entry points are bound, declared and exported."""
import os

import pytest

KERNELS = {"phk_chain_group_emit_kernel": 2, "phk_chain_group_backward_kernel": 3, "phk_chain_group_forward_kernel": 3,
           "phk_chain_group_viterbi_kernel": 3, "phk_chain_group_expect_kernel": 2, "phk_chain_group_fold_kernel": 1}
PER_RECORD = ("phk_chain_group_backward_kernel", "phk_chain_group_forward_kernel", "phk_chain_group_viterbi_kernel")
LDS_LIMIT = 160 * 1024
ENTRIES = ("phk_chain_set_groups", "phk_chain_set_grouped", "phk_chain_expect_grouped")


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_group_kernels_are_present_without_scratch_or_spills(resources):
    for kernel, variants in KERNELS.items():
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == variants, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
            assert 2 * r["lds_bytes"] <= LDS_LIMIT, (name, r)
            assert r["vgpr_count"] <= 256, (name, r)     # two waves per SIMD at the least
            if kernel in PER_RECORD:
                assert r["lds_bytes"] == 0, (name, r)


def test_no_group_kernel_counts_as_an_older_kernel(resources):
    from tests import test_chain_scan_resources as scan
    from tests import test_compose_resources as old
    older = list(old.KERNELS) + list(scan.KERNELS)
    group = [name for name in resources if "phk_chain_group_" in name]
    assert len(group) == sum(KERNELS.values()), sorted(group)
    for name in group:
        assert not any(k in name for k in older), name
    # and the older tests still find their kernels in the counts they expect
    for kernel, variants in list(old.KERNELS.items()) + list(scan.KERNELS.items()):
        assert len([name for name in resources if kernel in name]) == variants, kernel


def test_entry_points_and_constants():
    from phamers_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "phamers_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    for method in ("set_groups", "set_grouped", "expect_grouped"):
        assert hasattr(_lib.Chain, method), method
    assert lib.phk_abi_version() == _lib.ABI_VERSION == 2
