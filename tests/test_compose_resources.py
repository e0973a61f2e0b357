"""CPU-only: the kernels of the S-state chain (phamers_amd/csrc/chain.hip) are in the built library --
the per-record kernels once per padded state count (2, 4, 8), the two matrix-pipe kernels once per loader variant --, keep
nothing in scratch, spill nothing and use no LDS, and the entry points are bound and named in the header."""
import os

import pytest

KERNELS = {"phk_chain_emit_kernel": 2, "phk_chain_rowmax_kernel": 1, "phk_chain_backward_kernel": 3,
           "phk_chain_forward_kernel": 3, "phk_chain_viterbi_kernel": 3, "phk_chain_trace_kernel": 1,
           "phk_chain_spread_kernel": 1, "phk_chain_expect_kernel": 2, "phk_chain_fold_kernel": 1}
LDS_LIMIT = 160 * 1024
ENTRIES = ("phk_chain_create", "phk_batch_chain_create", "phk_chain_create_from_emissions", "phk_chain_set",
           "phk_chain_emissions", "phk_chain_expect", "phk_chain_decode", "phk_chain_grid_pass", "phk_chain_destroy")


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_chain_kernels_are_present_without_scratch_or_spills(resources):
    for kernel, variants in KERNELS.items():
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == variants, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
            assert 2 * r["lds_bytes"] <= LDS_LIMIT and r["lds_bytes"] == 0, (name, r)
            assert r["vgpr_count"] <= 256, (name, r)     # two waves per SIMD at the least


def test_entry_points_and_constants():
    from phamers_amd import _lib, compose
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "phamers_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert "#define PHK_CHAIN_MAX_STATES 8" in header and _lib.CHAIN_MAX_STATES == compose.MAX_STATES == 8
    assert lib.phk_chain_grid_pass() == 32768
    assert lib.phk_abi_version() == _lib.ABI_VERSION == 2
