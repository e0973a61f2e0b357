"""CPU-only: the kernels of the track segmentation (phamers_amd/csrc/segment.hip) are in the built
library, keep nothing in scratch and spill nothing, and two workgroups of the walk kernel (its 64 tiles' beta vectors, two
arrays of 64 x 65 doubles, and the tiles' places) fit a compute unit's 160 KiB of LDS."""
import os

import pytest

KERNELS = ("phk_seg_tile_kernel", "phk_seg_carry_kernel", "phk_seg_walk_kernel", "phk_seg_trace_kernel", "phk_seg_state_kernel")
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_segment_kernels_are_present_without_scratch_or_spills(resources):
    for kernel in KERNELS:
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == 1, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
            assert 2 * r["lds_bytes"] <= LDS_LIMIT, (name, r)
    walk = [r for name, r in resources.items() if "phk_seg_walk_kernel" in name][0]
    assert walk["lds_bytes"] == 2 * 64 * 65 * 8 + 64 * 8 + 64 * 4


def test_entry_points_and_constants():
    from phamers_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "phk_segment_decode") and hasattr(lib, "phk_segment_grid_pass")
    assert lib.phk_segment_grid_pass() % _lib.SEG_TILE == 0 and lib.phk_segment_grid_pass() >= 64 * _lib.SEG_TILE
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "phamers_hip.h")).read()
    assert "#define PHK_SEG_TILE %d\n" % _lib.SEG_TILE in header
    assert "#define PHK_SEG_QUANT_BITS %d\n" % _lib.SEG_QUANT_BITS in header
