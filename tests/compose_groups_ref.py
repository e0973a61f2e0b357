"""The statement of the grouped chain (phamers_amd/compose.py ``fit_groups``, csrc/chain.hip): the
records of a call are cut into groups of consecutive records and every group is a problem of its own.  So the grouped
E-step, the grouped decode and the grouped fit are, by definition, loops over the groups of what tests/compose_ref.py states
for one set of parameters and of ``compose.fit`` on the group's records alone:

    E-step   group g: ``compose_ref.StatementEStep`` on g's rows and g's own record offsets with g's parameters; an inactive
             group, and a group without windows, gives zeros
    decode   likewise ``StatementEStep.decode``; zeros for the groups passed over
    status   ``GROUP_TOO_SHORT`` (1) when g's records hold fewer than S blocks of ``block`` windows with k-mers (blocks never
             cross records; ``compose.fit`` raises ValueError for such rows), else ``GROUP_FITTED`` (0)
    fit      group g with status 0: ``compose.fit`` on g's rows alone; None otherwise
"""
import numpy as np

from tests import compose_ref as cref

GROUP_FITTED, GROUP_TOO_SHORT = 0, 1


def group_spans(offsets, group_offsets):
    """Per group (first record, last record + 1, first window, last window + 1)."""
    off, go = [int(o) for o in offsets], [int(g) for g in group_offsets]
    return [(r0, r1, off[r0], off[r1]) for r0, r1 in zip(go[:-1], go[1:])]


def group_rows(counts, offsets, group_offsets, g):
    """(rows, record offsets from 0) of group g alone."""
    r0, r1, w0, w1 = group_spans(offsets, group_offsets)[g]
    off = np.asarray([int(o) for o in offsets[r0:r1 + 1]], dtype=np.int64)
    return np.asarray(counts)[w0:w1], (off - off[0]).astype(np.uint64)


def status(counts, offsets, group_offsets, n_states, block=20):
    out = []
    for g in range(len(group_offsets) - 1):
        rows, off = group_rows(counts, offsets, group_offsets, g)
        P = cref.blocks(rows, off, block)
        out.append(GROUP_TOO_SHORT if int((P.sum(axis=1) > 0).sum()) < n_states else GROUP_FITTED)
    return np.array(out, dtype=np.int64)


class StatementGroupEStep(object):
    """What compose._estep_groups returns, as the loop over the groups of ``compose_ref.StatementEStep``.  ``calls`` keeps
    the active mask of every E-step (class-wide: a test clears it first)."""
    calls = []

    def __init__(self, counts_or_batch, offsets, group_offsets, n_states, batch_rows=0):
        self.host = np.ascontiguousarray(counts_or_batch, dtype=np.uint32)
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        self.group_offsets = np.asarray(group_offsets, dtype=np.uint64)
        self.n, self.D, self.S = self.host.shape[0], self.host.shape[1], int(n_states)
        self.G = len(self.group_offsets) - 1

    def counts(self):
        return self.host

    def _work(self, active):
        spans = group_spans(self.offsets, self.group_offsets)
        return [(g,) + spans[g] for g in range(self.G) if (active is None or active[g]) and spans[g][3] > spans[g][2]]

    def _alone(self, g):
        rows, off = group_rows(self.host, self.offsets, self.group_offsets, g)
        return cref.StatementEStep(rows, off, self.S)

    def __call__(self, log_profiles, trans, init, temper, active):
        type(self).calls.append(None if active is None else np.array(active, dtype=bool))
        G, S, D = self.G, self.S, self.D
        T, Ns, xi, g0, L = np.zeros((G, S, D)), np.zeros((G, S)), np.zeros((G, S, S)), np.zeros((G, S)), np.zeros(G)
        for g, r0, r1, w0, w1 in self._work(active):
            T[g], Ns[g], xi[g], g0[g], L[g] = self._alone(g)(log_profiles[g], trans[g], init[g], temper)
        return T, Ns, xi, g0, L

    def decode(self, log_profiles, trans, init, temper, active):
        state, post = np.zeros(self.n, dtype=np.uint8), np.zeros((self.n, self.S))
        le, ps = np.zeros(len(self.offsets) - 1), np.zeros(len(self.offsets) - 1, dtype=np.int64)
        for g, r0, r1, w0, w1 in self._work(active):
            state[w0:w1], post[w0:w1], le[r0:r1], ps[r0:r1] = self._alone(g).decode(log_profiles[g], trans[g], init[g], temper)
        return state, post, le, ps

    def close(self):
        pass


def fit_loop(compose, counts, offsets, group_offsets, n_states, block=20, init=None, **options):
    """[Composition or None per group]: ``compose.fit`` on every group's rows alone (``compose``: the module, with whatever
    E-step the caller has put in place), None where the status rule says too short."""
    st = status(counts, offsets, group_offsets, n_states, block)
    out = []
    for g in range(len(group_offsets) - 1):
        if st[g] != GROUP_FITTED:
            out.append(None)
            continue
        rows, off = group_rows(counts, offsets, group_offsets, g)
        out.append(compose.fit(rows, off, n_states, block=block, init=init[g] if isinstance(init, list) else init, **options))
    return out, st


COMPOSITION_ARRAYS = ("log_profiles", "trans", "init", "occupancy", "expected_counts", "trace")


def assert_same_composition(got, want, what=""):
    """Bit for bit: every array, n_iter, converged, bic."""
    assert (got is None) == (want is None), what
    if got is None:
        return
    for name in COMPOSITION_ARRAYS:
        assert np.array_equal(getattr(got, name), getattr(want, name)), (what, name)
    assert (got.n_iter, got.converged, got.temper, got.pseudocount) == (want.n_iter, want.converged, want.temper,
                                                                        want.pseudocount), what
    assert got.bic == want.bic or (np.isnan(got.bic) and np.isnan(want.bic)), what
