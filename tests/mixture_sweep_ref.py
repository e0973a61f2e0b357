"""The statement of the mixture sweep.  A cell (K, start i, fold f) IS ``mixture.fit`` on the
training rows with the float64 statement of tests/mixture_ref.py as its E-step; the held-out l_i ARE ``mixture_ref.e_step``
on the held-out rows.  ``StatementSweep`` stands where ``_lib.MixtureSweep`` stands: every job goes through
``mixture_ref.e_step(dtype=float64)`` on its own rows, alone.  ``patched`` puts the statements in the hooks' places."""
import contextlib

import numpy as np

from tests import mixture_ref as mref


class StatementSweep(object):
    """The NumPy stand-in of ``_lib.MixtureSweep`` (same calls, same shapes of the answers)."""

    def __init__(self, counts, row_sets):
        from phamers_amd.likelihood import _count_rows
        self.host = _count_rows(counts, "counts")
        self.sets = [np.asarray(s, dtype=np.int64) for s in row_sets]
        assert all(len(s) and (np.diff(s) > 0).all() and 0 <= s[0] and s[-1] < len(self.host) for s in self.sets)
        self.calls, self.jobs_per_call = 0, []

    def step(self, jobs, rows=False, _budget_bytes=0, expect=True):
        assert expect or rows
        jobs = list(jobs)
        self.calls += 1
        self.jobs_per_call.append(len(jobs))
        out = []
        for s, logp, logw in jobs:
            g = mref.e_step(self.host[self.sets[s]], logp, logw, np.float64)
            out.append(((g["T"], g["Nk"], float(g["L"])) if expect else (None, None, None)) + (g["l"] if rows else None,))
        return out

    def close(self):
        pass


def evaluate(positive_scores, negative_scores):
    """(ROC area, accuracy at threshold 0) in NumPy: the area as the Mann-Whitney statistic with ties at one half."""
    p, n = np.asarray(positive_scores, dtype=np.float64), np.asarray(negative_scores, dtype=np.float64)
    wins = (p[:, None] > n[None, :]).sum() + 0.5 * (p[:, None] == n[None, :]).sum()
    return float(wins) / (len(p) * len(n)), float((p >= 0).sum() + (n < 0).sum()) / (len(p) + len(n))


@contextlib.contextmanager
def patched(monkeypatch):
    """phamers_amd.mixture with the statements in the places of its three device hooks; yields the module and the list of
    the StatementSweep objects it made."""
    from phamers_amd import mixture
    made = []

    def device(counts, row_sets):
        made.append(StatementSweep(counts, row_sets))
        return made[-1]
    monkeypatch.setattr(mixture, "_estep", mref.StatementEStep)
    monkeypatch.setattr(mixture, "_sweep_device", device)
    monkeypatch.setattr(mixture, "_evaluate", evaluate)
    yield mixture, made


def cell(counts, train, K, seed, **kw):
    """The statement of one cell: ``fit`` on the training rows (``mixture._estep`` patched by the caller)."""
    from phamers_amd import mixture
    return mixture.fit(np.asarray(counts)[train], K, seed=seed, **kw)
