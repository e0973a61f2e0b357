"""CPU-only: the kernels of the stacked mixture E-step (phamers_amd/csrc/mixture_sweep.hip) are in the
built library -- the two products once per loader variant, the fold and the gather once --, keep nothing in scratch, spill
nothing and use no LDS; the single-table kernels of mixture.hip are there as often as before; the entry points are bound."""
import os

import pytest

from tests.test_mixture_resources import KERNELS as SINGLE_KERNELS

KERNELS = {"phk_mixsweep_resp_kernel": 2, "phk_mixsweep_expect_kernel": 2, "phk_mixsweep_fold_kernel": 1,
           "phk_mixsweep_gather_kernel": 1}
ENTRIES = ("phk_mix_sweep_create", "phk_batch_mix_sweep_create", "phk_mix_sweep_step", "phk_mix_sweep_destroy")


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_sweep_kernels_are_present_without_scratch_spills_or_lds(resources):
    for kernel, variants in KERNELS.items():
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == variants, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
            assert r["lds_bytes"] == 0 and r["vgpr_count"] <= 256, (name, r)     # two waves per SIMD: registers alone decide


def test_single_table_kernels_are_counted_as_before(resources):
    assert SINGLE_KERNELS == {"phk_mix_resp_kernel": 2, "phk_mix_expect_kernel": 2, "phk_mix_fold_kernel": 1}
    for kernel, variants in SINGLE_KERNELS.items():
        assert len([name for name in resources if kernel in name]) == variants, kernel
        assert not any(kernel in name for name in KERNELS)


def test_entry_points_and_abi():
    from phamers_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "phamers_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.phk_abi_version() == _lib.ABI_VERSION == 2
    assert hasattr(_lib.MixtureSweep, "step") and hasattr(_lib.MixtureSweep, "close")
