"""phamers_amd._lib's helpers that need no GPU: the draw packer of the batched k-means entry points and the close / __del__
pair every resident handle inherits, against a library that only records its calls."""
import numpy as np
import pytest

from phamers_amd import _lib


# ---- _pack_draws ---------------------------------------------------------------------------------------------------------
def test_pack_draws_offsets_and_order():
    ks = [3, 1, 8, 2]   # 3, 2, 4, 2 trials per centre: 6, 0, 28, 2 draws
    rng = np.random.RandomState(0)
    draws = [rng.uniform(size=(k - 1, _lib.kmeans_trials(k))) for k in ks]
    flat, offs = _lib._pack_draws(np.asarray(ks, dtype=np.uint32), draws)
    assert flat.dtype == np.float64 and flat.flags["C_CONTIGUOUS"] and offs.dtype == np.uint64
    assert offs.tolist() == [0, 6, 6, 34] and flat.size == 36
    for k, d, o in zip(ks, draws, offs):
        assert np.array_equal(flat[int(o):int(o) + d.size], d.ravel()), k


def test_pack_draws_pads_an_empty_result_to_one_element():
    for ks in ([1, 1, 1], []):
        flat, offs = _lib._pack_draws(ks, [np.zeros((0, 2))] * len(ks))
        assert flat.dtype == np.float64 and flat.tolist() == [0.0] and offs.tolist() == [0] * len(ks)


def test_pack_draws_names_the_problem_and_the_shape_it_wants():
    with pytest.raises(ValueError) as err:
        _lib._pack_draws([2, 8], [np.zeros((1, 2)), np.zeros((7, 3))])
    assert str(err.value) == "draws of problem 1 must be (7, 4)"
    _lib._pack_draws([0], [np.zeros(5)])   # k < 1 is the library's to refuse, with its own message


def test_trials_per_centre():
    assert [_lib.kmeans_trials(k) for k in (1, 2, 3, 7, 8, 54, 55, 8103, 8104)] == [2, 2, 3, 3, 4, 5, 6, 10, 11]


# ---- the resident handles ------------------------------------------------------------------------------------------------
DESTROY = {_lib.Model: "phk_model_destroy", _lib.Placement: "phk_placement_destroy", _lib.Sweep: "phk_sweep_destroy",
           _lib.ComboGrid: "phk_combo_grid_destroy", _lib.DbscanRows: "phk_dbscan_sweep_destroy", _lib.Batch: "phk_batch_free"}


class _RecordingLib(object):
    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name,) + args)
            if self.fail:
                raise RuntimeError("destroy failed")
            return 0
        return entry


class _FakeContext(object):
    def __init__(self, fail=False):
        self.lib, self.handle = _RecordingLib(fail), "ctx"


def _resident(cls, ctx):
    h = object.__new__(cls)   # (no device: the constructors are not run)
    h.ctx, h.handle = ctx, "handle"
    return h


@pytest.mark.parametrize("cls", list(DESTROY), ids=lambda c: c.__name__)
def test_closing_twice_destroys_once(cls):
    ctx = _FakeContext()
    h = _resident(cls, ctx)
    h._open()
    h.close()
    h.close()
    assert ctx.lib.calls == [(DESTROY[cls], "ctx", "handle")] and h.handle is None
    with pytest.raises(ValueError, match="this %s is closed" % cls.__name__):
        h._open()


@pytest.mark.parametrize("cls", list(DESTROY), ids=lambda c: c.__name__)
def test_closing_after_the_context_calls_nothing(cls):
    ctx = _FakeContext()
    h = _resident(cls, ctx)
    ctx.handle = None   # Context.close()
    h.close()
    h.__del__()
    assert ctx.lib.calls == [] and h.handle is None


@pytest.mark.parametrize("cls", list(DESTROY), ids=lambda c: c.__name__)
def test_collection_swallows_a_failing_destroy(cls):
    ctx = _FakeContext(fail=True)
    h = _resident(cls, ctx)
    h.__del__()
    assert ctx.lib.calls == [(DESTROY[cls], "ctx", "handle")]
    with pytest.raises(RuntimeError):
        _resident(cls, ctx).close()
