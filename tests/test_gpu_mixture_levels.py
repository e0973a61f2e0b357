"""GPU: the mixture E-step (mixture.hip) past one level of the fold tree, and N_k and L in the device's own order.

256 blocks of 1024 rows are the last shape the tree folds in one level, 257 the first that takes two (``mix_run`` then
ping-pongs between its two fold buffers).  N_k and L are plain float64 vector adds, so they are restated exactly from the
device's own r and l by ``mixture_ref.device_order`` (the slot rule of ``mix_expect_body``, then the tree) and compared bit
for bit; tests/test_mixture_host.py shows on the same inputs that every other order gives other bits.  T, N_k, L and l also
stay inside ``check_e_step``'s bound, which counts the levels.  Every test prints its wall time."""
import time

import numpy as np
import pytest

from tests import helpers, mixture_ref as mref
from tests.test_gpu_mixture import e_step, odd_width_rows, same, table_of

pytestmark = pytest.mark.gpu
RB = mref.BLOCK_ROWS
ONE_LEVEL, TWO_LEVELS = 256 * RB, 256 * RB + 1


@pytest.fixture(autouse=True)
def wall_time(request):
    start = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - start))


@pytest.fixture(scope="module")
def case():
    """dict(counts (TWO_LEVELS, 4), 1: (logp, logw), 2: (logp, logw)); the one-level shape is the first ONE_LEVEL rows."""
    counts, logp, logw = mref.two_profile_case(TWO_LEVELS, 2)
    return {"counts": counts, 1: mref.two_profile_case(TWO_LEVELS, 1)[1:], 2: (logp, logw)}


@pytest.fixture(scope="module")
def rows():
    """The ``rows`` fixture of tests/test_gpu_mixture.py: 2 * RB + 1 golden rows, phage and bacterial alternating."""
    g = helpers.load_npz("ref_features.npz")
    pos, neg = g["pos_counts"].astype(np.uint32), g["neg_counts"].astype(np.uint32)
    n = RB + 1
    out = np.empty((2 * n, 256), dtype=np.uint32)
    out[0::2], out[1::2] = pos[:n], neg[:n]
    return out[:2 * RB + 1]


def responsibilities(counts, logp, logw):
    from phamers_amd import _lib
    table = _lib.MixtureTable(_lib.get_context(), logp, logw)
    try:
        return table.responsibilities(counts)
    finally:
        table.close()


def assert_device_order(got, r, l):
    """N_k and L of ``got`` are the slot rule and the tree over the device's own r and l, bit for bit."""
    assert np.array_equal(l, got["l"])
    Nk, L = mref.device_order(r, l)
    assert np.array_equal(got["Nk"], Nk), (got["Nk"], Nk)
    assert got["L"] == L, (got["L"], L)


# ---- 1. 256 and 257 blocks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [ONE_LEVEL, TWO_LEVELS])
def test_one_component_is_exact_on_either_side_of_the_second_level(case, N):
    counts = case["counts"][:N]
    logp, logw = case[1]
    assert logw[0] == 0.0 and mref.tree_levels(-(-N // RB)) == (1 if N == ONE_LEVEL else 2)
    got = e_step(counts, logp, logw)
    assert np.array_equal(got["T"][0], counts.sum(axis=0, dtype=np.uint64).astype(np.float64))
    assert got["Nk"][0] == float(N) and (got["max_resp"] == 1.0).all() and (got["argmax"] == 0).all()
    assert got["L"] == mref.device_order(np.ones((N, 1)), got["l"])[1]


@pytest.mark.parametrize("N", [ONE_LEVEL, TWO_LEVELS])
def test_two_components_in_the_device_order_on_either_side_of_the_second_level(case, N):
    counts = case["counts"][:N]
    logp, logw = case[2]
    r, l = responsibilities(counts, logp, logw)
    got = e_step(counts, logp, logw)
    assert (got["Nk"] >= N / 8.0).all()
    assert_device_order(got, r, l)
    print("N=%d worst error / bound: %.4f" % (N, mref.check_e_step(got, counts, logp, logw)))


def test_two_levels_give_the_same_bits_for_any_split_entry_point_and_run(case):
    counts = case["counts"]
    logp, logw = case[2]
    whole = e_step(counts, logp, logw)
    assert same(whole, e_step(counts, logp, logw, resident=True))
    # three batches: the partial vectors of batches 1 and 2 and of batch 3 meet in the second level's one addition
    assert same(whole, e_step(counts, logp, logw, batch_rows=100 * RB))
    assert same(whole, e_step(counts, logp, logw, batch_rows=100 * RB, resident=True))
    assert same(whole, e_step(counts, logp, logw, batch_rows=0))
    assert same(whole, e_step(counts, logp, logw))             # run to run


# ---- 2. the order statement where a block edge cuts the four slots ---------------------------------------------------------
@pytest.mark.parametrize("N", [RB - 1, RB, RB + 1, 2 * RB + 1])
def test_device_order_at_the_block_edges(rows, N):
    counts = rows[:N]
    logp, logw = table_of(rows, 17)
    r, l = responsibilities(counts, logp, logw)
    assert_device_order(e_step(counts, logp, logw), r, l)


def test_device_order_at_a_width_that_goes_up_from_the_host():
    counts = odd_width_rows()
    logp, logw = table_of(counts, 7, seed=30)
    r, l = responsibilities(counts, logp, logw)
    assert_device_order(e_step(counts, logp, logw), r, l)
    assert_device_order(e_step(counts, logp, logw, batch_rows=RB), r, l)
