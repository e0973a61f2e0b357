"""The scenarios of tests/test_gpu_score_chain.py and tools/gen_golden_score_chain.py: small seeded batches that together take
the branches of the fast scorer's driver (phk_score_fast) and of the count -> score hand-over (phk_count_score_dev).  For each
scenario `run` returns what the fixture pins: the launches per kernel of the call's profile, score_stats_ex() and the SHA-256
of the score bytes and of the status word.  Test-only code."""
import hashlib

import numpy as np

from tests import helpers

BASES = np.frombuffer(b"ATGC", dtype=np.uint8)


def contigs(seed, lengths, skew=0.25):
    """Random contigs (uint8 ASCII arrays), each with a base composition of its own."""
    rng = np.random.default_rng(seed)
    out = []
    for L in lengths:
        p = 0.25 * (1.0 + skew * rng.uniform(-1.0, 1.0, 4))
        out.append(BASES[rng.choice(4, int(L), p=p / p.sum())])
    return out


def repeats(seed, n, L):
    """Low-complexity contigs: a motif of 3 .. 7 bases repeated to L bases -- a handful of k-mers hold every window."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        motif = BASES[rng.integers(0, 4, int(rng.integers(3, 8)))]
        out.append(np.tile(motif, L // len(motif) + 1)[:L])
    return out


class Input(object):
    """Sequences packed on the device, as phk_count_score_dev takes them."""

    def __init__(self, ctx, seqs):
        from phamers_amd import device
        self.n = len(seqs)
        offs = np.zeros(self.n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in seqs])
        self.T = int(offs[-1])
        d_bases = device.DeviceArray.from_host(ctx, np.ascontiguousarray(np.concatenate(seqs)))
        self.d_off = device.DeviceArray.from_host(ctx, offs)
        self.d_packed = device.DeviceArray(ctx, device.packed_words(self.T), np.uint32)
        d_mask = device.DeviceArray(ctx, device.mask_words(self.T), np.uint32)
        device.pack_ascii(ctx, d_bases, self.T, self.d_packed, d_mask)
        ctx.sync()
        d_bases.free()
        d_mask.free()

    def counts(self, ctx, k):
        from phamers_amd import device
        d = device.DeviceArray(ctx, (self.n, 4 ** k), np.uint32)
        device.count(ctx, self.d_packed, None, self.T, self.d_off, self.n, k, d)
        out = d.to_host()
        d.free()
        return out


def count_score(ctx, model, inp, k, method="combo"):
    """(counts, scores, status word) of one phk_count_score_dev call; the outputs start from garbage."""
    from phamers_amd import device
    d_counts = device.DeviceArray.from_host(ctx, np.full((inp.n, 4 ** k), 0xABCD, np.uint32))
    d_scores = device.DeviceArray.from_host(ctx, np.full(inp.n, 7.0))
    d_status = device.DeviceArray.from_host(ctx, np.full(1, 0x5A5A, np.uint32))
    device.count_score(ctx, model, inp.d_packed, None, inp.T, inp.d_off, inp.n, k, method, d_counts, d_scores, d_status)
    out = d_counts.to_host(), d_scores.to_host(), int(d_status.to_host()[0])
    for a in (d_counts, d_scores, d_status):
        a.free()
    return out


def score_rows(ctx, model, Q, method="combo"):
    """(scores, status word) of one phk_score_dev call on normalised float64 rows."""
    from phamers_amd import device
    d_q = device.DeviceArray.from_host(ctx, np.ascontiguousarray(Q, dtype=np.float64))
    d_scores = device.DeviceArray.from_host(ctx, np.full(len(Q), 7.0))
    d_status = device.DeviceArray.from_host(ctx, np.full(1, 0x5A5A, np.uint32))
    device.score(ctx, model, d_q, len(Q), method, d_scores, d_status)
    out = d_scores.to_host(), int(d_status.to_host()[0])
    for a in (d_q, d_scores, d_status):
        a.free()
    return out


# ---- models ---------------------------------------------------------------------------------------------------------------
def model_k4(ctx):
    from oracle import oracle
    from phamers_amd import _lib
    ref, g = helpers.load_npz("ref_features.npz"), helpers.load_npz("scoring_k4.npz")
    pos = oracle.normalize_counts(ref["pos_counts"].astype(np.int64))
    neg = oracle.normalize_counts(ref["neg_counts"].astype(np.int64))
    return _lib.Model(ctx, pos, neg, g["cpos_full"], g["cneg_full"], 3)


def genome_cluster(seed, L):
    """One GC-rich genome: a reference holds CLUSTER near-duplicates of its count row, queries cut from it find them all
    inside the two-digit int8 window."""
    rng = np.random.default_rng(seed)
    return BASES[rng.choice(4, L, p=[0.12, 0.13, 0.40, 0.35])]


CLUSTER = 12


def model_general(ctx, k, n_genomes, L, seed, cluster=None):
    """n_genomes random genomes of L bases, half of them positive; `cluster`: plus CLUSTER copies of that genome's row, copy c
    with c more windows of one k-mer, of alternating class."""
    from phamers_amd import _lib
    D = 4 ** k
    rows = Input(ctx, contigs(seed, [L] * n_genomes, skew=0.5)).counts(ctx, k).astype(np.float64)
    rows[: n_genomes // 2] *= 1.0 + 0.3 * np.sin(np.arange(D) * 0.37)
    labels = np.arange(n_genomes) < n_genomes // 2
    if cluster is not None:
        base = Input(ctx, [cluster]).counts(ctx, k).astype(np.float64)[0]
        extra = np.tile(base, (CLUSTER, 1))
        for c in range(CLUSTER):
            extra[c, (37 * c + 11) % D] += c
        rows = np.vstack((rows, extra))
        labels = np.append(labels, np.arange(CLUSTER) % 2 == 0)
    ref = rows / rows.sum(axis=1, keepdims=True)
    pos, neg = ref[labels], ref[~labels]
    cpos = np.stack([pos[i::6].mean(axis=0) for i in range(6)])
    cneg = np.stack([neg[i::6].mean(axis=0) for i in range(6)])
    return _lib.Model(ctx, pos, neg, cpos, cneg, 3)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def seqs_k4_plain(n=3000):
    return contigs(11, [3000] * (n - 4) + [2999, 3001, 3, 0])          # (the last two: no window at all -> NaN, flagged)


def seqs_k4_five_batches():
    return contigs(12, [2500] * 4500)                                   # score_batch = 1024: 4 full batches + 404 rows


def seqs_k4_second_chance():
    """Rows holding a count above 2048, which the fp16 count operand cannot carry: they take the second chance."""
    return contigs(13, [4000] * 1500) + repeats(14, 24, 40000) + contigs(15, [4000] * 500)


def seqs_k5_uniform():
    return contigs(16, [10000] * 2496 + [9999, 10001, 5, 4, 0, 64, 10000])


def seqs_k5_ragged(genome, n_repeats=40, n_pieces=10):
    """Ragged lengths (the sorted slot kernel counts: the scorer prepares its operand), n_repeats low-complexity rows beyond the
    int8 operand and n_pieces pieces of the cluster's genome, whose two-digit windows hold the whole cluster.  Each kind
    fills one hand-over queue of the first pass: a queue of at least 32 rows (PHK_SUBPASS_MIN) is swept as a sub-batch --
    the rows beyond the operand by the f16 kernel, the wide windows by the three-digit int8 sweep -- a shorter one is
    appended to the brute-force queue.  40 + 10 takes one pair of these branches, 5 + 40 the other."""
    rng = np.random.default_rng(17)
    lens = np.minimum((rng.pareto(1.1, 1500) * 2000).astype(np.int64) + 200, 60000)
    pieces = [genome[s:s + 10000] for s in np.linspace(0, 90000, n_pieces).astype(int)]
    return contigs(18, lens) + repeats(19, n_repeats, 20000) + pieces


def seqs_k6():
    return contigs(20, [6000] * 2100)      # (with 17 blocks of columns: enough for the sweep's two column groups and their merge)


# ---- the scenarios --------------------------------------------------------------------------------------------------------
def digest(launch_fn, ctx):
    """Runs `launch_fn` (-> scores, status word) under the kernel profile."""
    ctx.sync()
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        scores, status = launch_fn()
    finally:
        ctx.profile_enable(False)
    return {"launches": {name: int(v[1]) for name, v in sorted(ctx.profile().items())},
            "stats": ctx.score_stats_ex(),
            "scores_sha256": hashlib.sha256(np.ascontiguousarray(scores).tobytes()).hexdigest(),
            "status_sha256": hashlib.sha256(np.uint32(status).tobytes()).hexdigest()}


class Scenarios(object):
    """Builds models and inputs once; `run(name)` -> the digest of scenario `name` (NAMES, in any order)."""

    NAMES = (["k4 one batch %s" % m for m in ("knn", "kmeans", "combo")] +
             ["k4 five batches tail aside", "k4 five batches one stream", "k4 second chance", "k4 float64 rows",
              "k4 column mask", "k5 count score", "k5 ragged", "k5 counts in"] +
             ["k5 proposal %s" % p for p in ("cxf", "i83", "hi")] + ["k6", "k4 rerank w", "k4 rerank g", "k5 rerank w", "k5 ragged wide"])

    def __init__(self, ctx):
        self.ctx = ctx
        self.m4 = model_k4(ctx)
        self.genome = genome_cluster(30, 100000)
        self.m5 = model_general(ctx, 5, 150, 30000, 31, cluster=self.genome)
        self.m6 = model_general(ctx, 6, 528, 20000, 32)
        self.inputs = {}

    def close(self):
        for m in (self.m4, self.m5, self.m6):
            m.close()

    def input(self, key, make):
        if key not in self.inputs:
            self.inputs[key] = Input(self.ctx, make())
        return self.inputs[key]

    def run(self, name):
        ctx = self.ctx
        opts, model, k, method = {}, self.m4, 4, "combo"
        if name.startswith("k4 one batch"):
            inp, method = self.input("k4", seqs_k4_plain), name.split()[-1]
        elif name.startswith("k4 five batches"):
            inp = self.input("k4x5", seqs_k4_five_batches)
            opts = {"score_batch": ("1024", "0"), "tail_aside": ("1" if name.endswith("aside") else "0", "1")}
        elif name == "k4 second chance":
            inp = self.input("k4sc", seqs_k4_second_chance)
        elif name == "k4 float64 rows" or name.startswith("k4 rerank"):
            # the split-query lists at k = 4 are where the driver reads the `rerank` option (launch_rerank): 'w' one wave per
            # query, 'g' four queries per wave for every query, else the lane-per-query decision kernel first
            c = self.input("k4", seqs_k4_plain).counts(ctx, 4)[:-2].astype(np.float64)
            Q = c / c.sum(axis=1, keepdims=True)
            with ctx.options(**({"rerank": (name.split()[-1], "")} if "rerank" in name else {})):
                return digest(lambda: score_rows(ctx, model, Q), ctx)
        elif name == "k4 column mask":
            inp = self.input("k4", seqs_k4_plain)
            mask = np.zeros(len(model._pos) + len(model._neg), dtype=bool)
            mask[::3] = True
            model.set_column_mask(mask)
            try:
                return digest(lambda: count_score(ctx, model, inp, 4)[1:], ctx)
            finally:
                model.set_column_mask(None)
        elif name == "k5 count score":
            inp, model, k = self.input("k5", seqs_k5_uniform), self.m5, 5
        elif name == "k5 ragged":
            inp, model, k = self.input("k5r", lambda: seqs_k5_ragged(self.genome)), self.m5, 5
        elif name == "k5 ragged wide":
            inp, model, k = self.input("k5rw", lambda: seqs_k5_ragged(self.genome, n_repeats=5, n_pieces=40)), self.m5, 5
        elif name == "k5 rerank w":       # general D: no lane-per-query decision kernel, no pending centroid distances
            inp, model, k, opts = self.input("k5", seqs_k5_uniform), self.m5, 5, {"rerank": ("w", "")}
        elif name == "k5 counts in":      # count rows without row sums: the driver computes them
            from phamers_amd import device
            c = self.input("k5", seqs_k5_uniform).counts(ctx, 5)

            def call():
                d_c, d_s = device.DeviceArray.from_host(ctx, c), device.DeviceArray.from_host(ctx, np.full(len(c), 7.0))
                d_st = device.DeviceArray.from_host(ctx, np.full(1, 0x5A5A, np.uint32))
                device.score_counts(ctx, self.m5, d_c, len(c), "combo", d_s, d_st)
                out = d_s.to_host(), int(d_st.to_host()[0])
                for a in (d_c, d_s, d_st):
                    a.free()
                return out
            return digest(call, ctx)
        elif name.startswith("k5 proposal"):
            inp, model, k = self.input("k5", seqs_k5_uniform), self.m5, 5
            opts = {"proposal": (name.split()[-1], "")}
        elif name == "k6":
            inp, model, k = self.input("k6", seqs_k6), self.m6, 6
        else:
            raise KeyError(name)
        with ctx.options(**opts):
            return digest(lambda: count_score(ctx, model, inp, k, method)[1:], ctx)
