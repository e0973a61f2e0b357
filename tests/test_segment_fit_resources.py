"""CPU-only: the kernels of the segmentation fit (phamers_amd/csrc/segment.hip) are in the built
library once each, keep nothing in scratch and spill nothing, two workgroups of the xi kernel (its 64 tiles' beta vectors, two
arrays of 64 x 64 doubles) fit a compute unit's 160 KiB of LDS as the walk kernel's do, and the entry points are bound."""
import os

import pytest

KERNELS = ("phk_seg_fb_carry_kernel", "phk_seg_xi_kernel", "phk_seg_fold_kernel", "phk_seg_reduce_kernel")
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_fit_kernels_are_present_without_scratch_or_spills(resources):
    for kernel in KERNELS:
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == 1, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
            assert 2 * r["lds_bytes"] <= LDS_LIMIT, (name, r)
    xi = [r for name, r in resources.items() if "phk_seg_xi_kernel" in name][0]
    assert xi["lds_bytes"] == 2 * 64 * 64 * 8
    reduce = [r for name, r in resources.items() if "phk_seg_reduce_kernel" in name][0]
    assert reduce["lds_bytes"] == 7 * 256 * 8


def test_entry_points_and_constants():
    from phamers_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "phk_segment_expect") and hasattr(lib, "phk_segment_fit")
    assert "phk_segment_expect" in _lib.SIGNATURES and "phk_segment_fit" in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "phamers_hip.h")).read()
    for name, value in (("PHK_SEG_TRACE_COLS", _lib.SEG_TRACE_COLS), ("PHK_SEG_START_FIXED", _lib.SEG_START_FIXED),
                        ("PHK_SEG_START_FREE", _lib.SEG_START_FREE), ("PHK_SEG_START_STATIONARY", _lib.SEG_START_STATIONARY)):
        assert "#define %s %d\n" % (name, value) in header
    for name, value in (("PHK_SEG_FIT_MAX_ITER", _lib.SEG_FIT_MAX_ITER), ("PHK_SEG_FIT_CONVERGED", _lib.SEG_FIT_CONVERGED),
                        ("PHK_SEG_FIT_CLAMPED", _lib.SEG_FIT_CLAMPED), ("PHK_SEG_FIT_NO_TRANSITIONS", _lib.SEG_FIT_NO_TRANSITIONS)):
        assert "#define %s %du\n" % (name, value) in header
