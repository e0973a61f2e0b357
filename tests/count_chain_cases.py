"""The scenarios of tests/test_gpu_count_chain.py and tools/gen_golden_count_chain.py: small seeded batches that together take
the branches of the count launcher (phk_launch_count: count_route, csrc/count_shared.h).  For each scenario `run` returns what
the fixture pins: the launches per kernel of the call's profile and the SHA-256 of the count bytes and of the window totals
(`nwin`).  Test-only code."""
import hashlib

import numpy as np

from tests.score_chain_cases import contigs

N_CODE = ord("N")


def with_invalid(seqs, seed, per_contig=3):
    """A few bases of every contig replaced by N: the batch then needs its validity mask."""
    rng = np.random.default_rng(seed)
    out = []
    for s in seqs:
        s = s.copy()
        if len(s):
            s[rng.integers(0, len(s), per_contig)] = N_CODE
        out.append(s)
    return out


def seqs_uniform():
    return contigs(51, [2500] * 300)


def ragged_lengths(k=4):
    """200 heavy-tailed lengths, three of them above 2 x 32768 + k windows: cut into pieces by a sorted batch."""
    from phamers_amd import synth
    lens = synth.ragged_lengths(15, 200, lo=300, hi=400000, shape=0.9)
    lens[3], lens[10], lens[11] = 0, k - 1, k
    lens[20], lens[30], lens[40] = 150000, 98304 + k - 1, 65536 + k
    return lens


def seqs_ragged():
    return contigs(52, ragged_lengths())


def seqs_tiny():
    return contigs(53, [300, 5, 600])       # 1024 bases at the most: the slot path is not taken


def seqs_empty():
    return contigs(54, [0, 0, 0])


class Input(object):
    """Sequences packed on the device with their validity mask, as phk_count_dev takes them."""

    def __init__(self, ctx, seqs):
        from phamers_amd import device
        self.n = len(seqs)
        offs = np.zeros(self.n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in seqs])
        self.T = int(offs[-1])
        self.d_off = device.DeviceArray.from_host(ctx, offs)
        self.d_packed = device.DeviceArray(ctx, device.packed_words(self.T), np.uint32)
        self.d_mask = device.DeviceArray(ctx, device.mask_words(self.T), np.uint32)
        if self.T:
            d_bases = device.DeviceArray.from_host(ctx, np.ascontiguousarray(np.concatenate(seqs)))
            device.pack_ascii(ctx, d_bases, self.T, self.d_packed, self.d_mask)
            ctx.sync()
            d_bases.free()


def count(ctx, inp, k, masked, n=None):
    """(counts, nwin) of one phk_count_dev call; both outputs start from garbage."""
    from phamers_amd import device
    rows = max(inp.n, 1)
    d_counts = device.DeviceArray.from_host(ctx, np.full((rows, 4 ** k), 0xABCD, np.uint32))
    d_nwin = device.DeviceArray.from_host(ctx, np.full(rows, 0xABCD, np.uint32))
    device.count(ctx, inp.d_packed, inp.d_mask if masked else None, inp.T, inp.d_off, inp.n if n is None else n, k, d_counts, d_nwin)
    out = d_counts.to_host(), d_nwin.to_host()
    d_counts.free()
    d_nwin.free()
    return out


def digest(launch_fn, ctx):
    """Runs `launch_fn` (-> counts, nwin) under the kernel profile."""
    ctx.sync()
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        counts, nwin = launch_fn()
    finally:
        ctx.profile_enable(False)
    return {"launches": {name: int(v[1]) for name, v in sorted(ctx.profile().items())},
            "counts_sha256": hashlib.sha256(np.ascontiguousarray(counts).tobytes()).hexdigest(),
            "nwin_sha256": hashlib.sha256(np.ascontiguousarray(nwin).tobytes()).hexdigest()}


INPUTS = {"uniform": seqs_uniform, "uniform N": lambda: with_invalid(seqs_uniform(), 61), "ragged": seqs_ragged,
          "ragged N": lambda: with_invalid(seqs_ragged(), 62), "tiny": seqs_tiny, "empty": seqs_empty}

# name -> (input, k, masked, options as {key: (value, restore)})
CASES = {
    "uniform k4": ("uniform", 4, False, {}),
    "uniform k4 masked": ("uniform N", 4, True, {}),
    "uniform k3": ("uniform", 3, False, {}),
    "uniform k5": ("uniform", 5, False, {}),
    "uniform k5 masked": ("uniform N", 5, True, {}),
    "ragged k4": ("ragged", 4, False, {}),
    "ragged k5 masked": ("ragged N", 5, True, {}),
    "ragged k4 unsorted": ("ragged", 4, False, {"count_sort": ("0", "1")}),
    "tiny k4": ("tiny", 4, False, {}),
    "uniform k2": ("uniform", 2, False, {}),
    "uniform k6": ("uniform", 6, False, {}),
    "empty k4": ("empty", 4, False, {}),
}
for _c in "0fqQpPdD2":          # ('2': a character that names nothing)
    CASES["uniform k4 lanes %s" % _c] = ("uniform", 4, False, {"count_lanes": (_c, "")})
for _c in "dD":
    CASES["uniform k5 lanes %s" % _c] = ("uniform", 5, False, {"count_lanes": (_c, "")})
SPECIAL = ["no contigs k4", "batch from ascii k4"]


class Scenarios(object):
    """Packs the inputs once; `run(name)` -> the digest of scenario `name` (NAMES, in any order)."""

    NAMES = list(CASES) + SPECIAL

    def __init__(self, ctx):
        self.ctx = ctx
        self.inputs = {}

    def input(self, key):
        if key not in self.inputs:
            self.inputs[key] = Input(self.ctx, INPUTS[key]())
        return self.inputs[key]

    def call(self, name):
        """(counts, nwin) of scenario `name`, outside the profile."""
        ctx = self.ctx
        if name == "no contigs k4":       # n = 0: nothing is touched, the garbage stays
            return count(ctx, self.input("tiny"), 4, False, n=0)
        if name == "batch from ascii k4":
            from phamers_amd import _lib
            b = _lib.Batch.from_sequences(ctx, [s.tobytes().decode("ascii") for s in seqs_uniform()], 4)
            try:
                return b.counts_u32(), b.row_sums()
            finally:
                b.close()
        key, k, masked, opts = CASES[name]
        with ctx.options(**opts):
            return count(ctx, self.input(key), k, masked)

    def run(self, name):
        self.input(CASES[name][0] if name in CASES else "tiny")     # (packed outside the profile)
        return digest(lambda: self.call(name), self.ctx)
