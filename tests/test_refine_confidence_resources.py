"""CPU-only: the kernel of the boundary confidence (phamers_amd/csrc/refine.hip) is in the built
library in its two variants -- the difference row in LDS, the two rows read from global memory --, keeps nothing in scratch,
spills no vector register, holds the LDS of the refinement kernel and leaves three waves to a SIMD; it does not count as a
``phk_refine_`` kernel (tests/test_refine_resources.py counts those); the entry points are bound, declared and exported; the
ABI version is 2.

Read after the build for gfx950:153 vector registers and 32 KiB of LDS with the table, 139 and none without; 5 and 6
scalar registers kept in lanes of a vector register (no memory behind them)."""
import os

import pytest

KERNELS = {"phk_boundary_confidence_kernel": 2}
LDS_LIMIT = 160 * 1024
ENTRIES = ("phk_refine_confidence_ascii", "phk_refine_confidence_fasta")


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_confidence_kernels_are_present_without_scratch_or_spills(resources):
    for kernel, variants in KERNELS.items():
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == variants, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
            assert 2 * r["lds_bytes"] <= LDS_LIMIT, (name, r)
            assert r["vgpr_count"] <= 168, (name, r)      # 256 threads: three waves per SIMD at the least
    table = [r for name, r in resources.items() if "phk_boundary_confidence_kernelILb1E" in name]
    direct = [r for name, r in resources.items() if "phk_boundary_confidence_kernelILb0E" in name]
    assert len(table) == 1 and len(direct) == 1
    assert table[0]["lds_bytes"] == 4 * 1024 * 8          # four waves x 1024 int64 differences, as the refinement kernel's
    assert direct[0]["lds_bytes"] == 0


def test_the_refinement_kernels_are_what_they_were(resources):
    from tests import test_refine_resources as old
    assert not any("phk_refine_" in name for name in resources if "phk_boundary_confidence_kernel" in name)
    for kernel, variants in old.KERNELS.items():
        assert len([name for name in resources if kernel in name]) == variants
    assert len([name for name in resources if "phk_refine_" in name]) == sum(old.KERNELS.values())


def test_entry_points_and_constants():
    from phamers_amd import _lib, compose, refine
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "phamers_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert hasattr(_lib, "refine_confidence") and hasattr(refine, "confidence") and hasattr(compose, "write_confidence_file")
    assert refine.DEFAULT_DROP == 3.0
    assert lib.phk_abi_version() == _lib.ABI_VERSION == 2
