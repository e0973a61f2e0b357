"""CPU-only: the kernel of the boundary refinement (phamers_amd/csrc/refine.hip) is in the built library
in its two variants -- the difference row in LDS, the two rows read from global memory --, keeps nothing in scratch and spills
nothing, and two of its workgroups fit the LDS of a CU; no ``phk_refine_`` kernel counts as one of the kernels the older
resource tests count by substring; the entry points are bound, declared and exported; the ABI version is 2."""
import glob
import importlib
import os

import pytest

KERNELS = {"phk_refine_boundaries_kernel": 2}
LDS_LIMIT = 160 * 1024
ENTRIES = ("phk_refine_boundaries_ascii", "phk_refine_boundaries_fasta", "phk_refine_grid_pass")


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_refine_kernels_are_present_without_scratch_or_spills(resources):
    for kernel, variants in KERNELS.items():
        found = {name: r for name, r in resources.items() if kernel in name}
        assert len(found) == variants, (kernel, sorted(found))
        for name, r in found.items():
            assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
            assert 2 * r["lds_bytes"] <= LDS_LIMIT, (name, r)
            assert r["vgpr_count"] <= 128, (name, r)      # 256 threads: four waves per SIMD at the least
    table = [r for name, r in resources.items() if "phk_refine_boundaries_kernelILb1E" in name]
    direct = [r for name, r in resources.items() if "phk_refine_boundaries_kernelILb0E" in name]
    assert len(table) == 1 and len(direct) == 1
    assert table[0]["lds_bytes"] == 4 * 1024 * 8          # four waves x 1024 int64 differences
    assert direct[0]["lds_bytes"] == 0
    assert len([name for name in resources if "phk_refine_" in name]) == sum(KERNELS.values())


def _older_tables():
    """The KERNELS / KERNEL tables of every other resource test, by module name."""
    here = os.path.dirname(os.path.abspath(__file__))
    tables = {}
    for path in sorted(glob.glob(os.path.join(here, "test_*_resources.py"))):
        module = os.path.splitext(os.path.basename(path))[0]
        if module == "test_refine_resources":
            continue
        m = importlib.import_module("tests." + module)
        names = getattr(m, "KERNELS", None)
        if names is None and hasattr(m, "KERNEL"):
            names = (m.KERNEL,)
        if names is not None:
            tables[module] = names
    return tables


def test_no_refine_kernel_counts_as_an_older_kernel(resources):
    tables = _older_tables()
    assert {"test_compose_resources", "test_chain_scan_resources", "test_compose_groups_resources", "test_mixture_resources",
            "test_segment_resources", "test_hosts_resources"} <= set(tables)
    mine = [name for name in resources if "phk_refine_" in name]
    for module, names in tables.items():
        for kernel in names:
            assert not any(kernel in name for name in mine), (module, kernel)
        # and the older tests still find their kernels in the counts they expect
        if isinstance(names, dict):
            for kernel, variants in names.items():
                assert len([name for name in resources if kernel in name]) == variants, (module, kernel)
    # the neighbour lookup has a kernel with "refine" in its name: neither name holds the other
    assert all("phk_nn_refine_kernel" not in name for name in mine)


def test_entry_points_and_constants():
    from phamers_amd import _lib, refine
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "phamers_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert hasattr(_lib, "refine_boundaries") and hasattr(refine, "boundaries")
    assert _lib.refine_grid_pass() == 2048 * 4
    assert lib.phk_abi_version() == _lib.ABI_VERSION == 2
