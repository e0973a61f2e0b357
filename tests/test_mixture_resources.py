"""CPU-only: the kernels of the mixture E-step (phamers_amd/csrc/mixture.hip) are in the built library
-- the two products once per loader variant, the fold once --, keep nothing in scratch and spill nothing, use no LDS (so two
workgroups per compute unit are limited by registers alone), and the entry points are bound."""
import os

import pytest

KERNELS = {"phk_mix_resp_kernel": 2, "phk_mix_expect_kernel": 2, "phk_mix_fold_kernel": 1}
LDS_LIMIT = 160 * 1024
ENTRIES = ("phk_mix_table_create", "phk_mix_table_update", "phk_mix_table_destroy", "phk_mix_block_rows", "phk_mix_expect",
           "phk_batch_mix_expect", "phk_mix_responsibilities", "phk_batch_mix_responsibilities")


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_mixture_kernels_are_present_without_scratch_or_spills(resources):
    for kernel, variants in KERNELS.items():
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == variants, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
            assert 2 * r["lds_bytes"] <= LDS_LIMIT and r["lds_bytes"] == 0, (name, r)


def test_entry_points_and_constants():
    from phamers_amd import _lib
    from tests import mixture_ref
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "phamers_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.phk_mix_block_rows() == mixture_ref.BLOCK_ROWS
    assert lib.phk_abi_version() == _lib.ABI_VERSION == 2
    assert _lib.MIX_MAX_COMPONENTS == 256
