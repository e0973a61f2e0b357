"""NumPy restatement of the integer ROC method of phamers_amd/csrc/evaluate.hip (phk_roc_curve): scikit-learn's
roc_curve(labels, scores, drop_intermediate=flag) with the counts kept as integers until the last step.

    roc_points(scores, labels, drop)     -> fps, tps (uint64), thresholds (float64), area2 (Python int = 2 P N AUC)
    rates(fps, tps, area2)               -> fpr, tpr, auc
    predictor_performance(pos, neg)      -> fpr, tpr, auc   (scripts/learning.py:185-196)
    truth_counts / truth_table / metrics -> scripts/learning.py:199-243
"""
import numpy as np

METRIC_NAMES = ('tp', 'fp', 'fn', 'tn', 'tpr', 'fpr', 'fnr', 'tnr', 'ppv', 'npv', 'fdr', 'acc')


def roc_points(scores, labels, drop_intermediate=True):
    scores = np.asarray(scores, dtype=np.float64).ravel()
    labels = (np.asarray(labels).ravel() != 0)
    if not np.isfinite(scores).all():
        raise ValueError("Input contains NaN or infinity.")
    n = len(scores)
    if n == 0:
        return np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.array([np.inf]), 0
    order = np.argsort(-(scores + 0.0), kind='stable')          # descending, ties in index order (+ 0.0: -0.0 -> +0.0)
    s, lab = scores[order], labels[order].astype(np.int64)
    marks = np.r_[np.flatnonzero(s[1:] != s[:-1]), n - 1]        # the last element of every run of equal scores
    tps = np.cumsum(lab)[marks]
    fps = 1 + marks - tps
    thr = s[marks]
    if drop_intermediate and len(fps) > 2:
        keep = np.r_[True, (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0), True]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    fps, tps, thr = np.r_[0, fps], np.r_[0, tps], np.r_[np.inf, thr]
    widths, heights = np.diff(fps), tps[1:] + tps[:-1]
    if 2 * int(fps[-1]) * int(tps[-1]) < 2 ** 63:                # (the sum is at most 2 P N: exact in int64 then)
        area2 = int(np.dot(widths.astype(np.int64), heights.astype(np.int64)))
    else:
        area2 = int(np.sum(widths.astype(object) * heights.astype(object)))
    return fps.astype(np.uint64), tps.astype(np.uint64), thr, area2


def rates(fps, tps, area2):
    fps, tps = np.asarray(fps, dtype=np.float64), np.asarray(tps, dtype=np.float64)
    n_neg, n_pos = int(fps[-1]), int(tps[-1])
    fpr = fps / fps[-1] if n_neg else np.full(fps.shape, np.nan)
    tpr = tps / tps[-1] if n_pos else np.full(tps.shape, np.nan)
    auc = int(area2) / (2 * n_pos * n_neg) if n_pos and n_neg else float('nan')
    return fpr, tpr, auc


def stack(positive_scores, negative_scores):
    pos, neg = np.asarray(positive_scores, dtype=np.float64).ravel(), np.asarray(negative_scores, dtype=np.float64).ravel()
    return np.concatenate((pos, neg)), np.r_[np.ones(len(pos), np.uint8), np.zeros(len(neg), np.uint8)]


def predictor_performance(positive_scores, negative_scores):
    fps, tps, _, area2 = roc_points(*stack(positive_scores, negative_scores))
    return rates(fps, tps, area2)


def truth_counts(positive_scores, negative_scores, threshold=0):
    pos, neg = np.asarray(positive_scores, dtype=np.float64), np.asarray(negative_scores, dtype=np.float64)
    return (int(np.sum(pos >= threshold)), int(np.sum(neg >= threshold)), int(np.sum(pos < threshold)),
            int(np.sum(neg < threshold)))


def truth_table(tp, fp, fn, tn):
    tpr = float(tp) / (tp + fn) if tp + fn != 0 else 0
    fpr = float(fp) / (fp + tn) if fp + tn != 0 else 0
    return tpr, fpr, 1 - tpr, 1 - fpr


def metrics(positive_scores, negative_scores, threshold=0):
    """The twelve values of scripts/learning.py:223-243 in METRIC_NAMES order (floats)."""
    tp, fp, fn, tn = (float(c) for c in truth_counts(positive_scores, negative_scores, threshold))
    tpr, fpr, fnr, tnr = truth_table(tp, fp, fn, tn)
    ppv, npv = tp / (tp + fp), tn / (tn + fn)
    return [tp, fp, fn, tn, tpr, fpr, fnr, tnr, ppv, npv, 1 - ppv, (tp + tn) / (tp + fp + fn + tn)]


# ---- the small cases shared by tools/gen_golden_evaluate.py and the tests (seeded; the inputs are not stored) ---------------
TILE = 4096   # PHK_SORT_TILE


def cases():
    """name -> (positive scores, negative scores)."""
    rng = np.random.RandomState(20)
    out = {}
    out["normal"] = (rng.normal(1, 1, 1500), rng.normal(0, 1, 2000))
    out["pm1"] = (rng.choice([-1.0, 1.0], 900, p=[0.2, 0.8]), rng.choice([-1.0, 1.0], 1100, p=[0.7, 0.3]))
    out["combo"] = (rng.choice([-1.0, 1.0], 700, p=[0.2, 0.8]) + np.tanh(rng.normal(0.5, 1, 700)),
                    rng.choice([-1.0, 1.0], 800, p=[0.7, 0.3]) + np.tanh(rng.normal(-0.5, 1, 800)))
    a, b = np.round(rng.normal(0.2, 0.5, 600), 1), np.round(rng.normal(-0.2, 0.5, 650), 1)
    a[a == 0] = np.where(rng.rand(int((a == 0).sum())) < 0.5, -0.0, 0.0)
    b[b == 0] = np.where(rng.rand(int((b == 0).sum())) < 0.5, -0.0, 0.0)
    a[:2], b[:2] = [-0.0, 0.0], [0.0, -0.0]
    out["rounded"] = (a, b)
    out["subnormal"] = (np.r_[rng.choice([5e-324, 1e-310, -5e-324, 2.5e-308], 300), 1.7 + 1e-16 * rng.randint(0, 9, 300)],
                        np.r_[rng.choice([5e-324, -1e-310, 0.0], 300), 1.7 - 1e-16 * rng.randint(0, 9, 200)])
    out["equal"] = (np.full(300, 0.25), np.full(500, 0.25))
    out["separated"] = (rng.uniform(1, 2, 400), rng.uniform(-2, -1, 300))
    out["inverted"] = (rng.uniform(-2, -1, 400), rng.uniform(1, 2, 300))
    out["one_one"] = (np.array([0.5]), np.array([-0.5]))
    out["two_tied"] = (np.array([0.5]), np.array([0.5]))
    out["one_many"] = (np.array([0.3]), rng.normal(0, 1, 999))
    out["many_one"] = (rng.normal(0, 1, 999), np.array([0.3]))
    for name, n in (("tile_minus", TILE - 1), ("tile", TILE), ("tile_plus", TILE + 1), ("tiles_rem", 3 * TILE + 77)):
        out[name] = (rng.normal(0.5, 1, n // 3), np.round(rng.normal(0, 1, n - n // 3), 3))
    return out


def case_thresholds(pos, neg):
    """0, a tied score value (one both classes hold, else any score), beyond both ends."""
    both = np.intersect1d(pos, neg)
    tied = float(both[len(both) // 2]) if len(both) else float(pos[0])
    lo, hi = min(pos.min(), neg.min()), max(pos.max(), neg.max())
    return [0.0, tied, float(lo - 1.0), float(hi + 1.0)]
