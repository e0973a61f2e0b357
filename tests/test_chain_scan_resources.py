"""CPU-only: the kernels of the chain's tile scan (phamers_amd/csrc/chain.hip) are in the built
library -- the per-tile and per-record kernels once per padded state count (2, 4, 8) --, keep nothing in scratch, spill
nothing and leave room for two workgroups' LDS on a CU; the three entry points are bound and named in the header."""
import os

import pytest

KERNELS = {"phk_chain_scan_tile_kernel": 3, "phk_chain_scan_carry_kernel": 3, "phk_chain_scan_walk_kernel": 3,
           "phk_chain_scan_path_kernel": 3, "phk_chain_scan_fold_kernel": 1, "phk_chain_scan_ends_kernel": 1,
           "phk_chain_scan_fill_kernel": 1}
LDS_LIMIT = 160 * 1024
ENTRIES = ("phk_chain_set_scan", "phk_chain_tile", "phk_chain_scan_grid_pass")


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_scan_kernels_are_present_without_scratch_or_spills(resources):
    for kernel, variants in KERNELS.items():
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == variants, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
            assert 2 * r["lds_bytes"] <= LDS_LIMIT, (name, r)
            assert r["vgpr_count"] <= 256, (name, r)     # two waves per SIMD at the least


def test_no_scan_kernel_counts_as_a_per_record_kernel(resources):
    from tests import test_compose_resources as old
    for name in resources:
        if "phk_chain_scan_" in name:
            assert not any(k in name for k in old.KERNELS), name


def test_entry_points_and_constants():
    from phamers_amd import _lib
    from tests import chain_scan_ref as sref
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "phamers_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert hasattr(_lib.Chain, "set_scan")
    assert "#define PHK_CHAIN_TILE 64" in header and lib.phk_chain_tile() == sref.TILE == 64
    assert lib.phk_chain_scan_grid_pass() == 4096
    assert lib.phk_abi_version() == _lib.ABI_VERSION == 2
