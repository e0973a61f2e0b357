"""The statement of the boundary refinement in Python ints, and ``compose.boundary_plan`` restated as
a plain loop.  No NumPy arithmetic touches a sum.

A sequence of L bases; the k-mer starting at base i is valid when i + k <= L and its k bases are symbols; code(i) is its column
in a count row (``kmer.count_string``: the first base is the most significant base-4 digit).  For a boundary
(seq, lo, x, hi, left_row, right_row) and a table q of ints:

    d(i) = q[left_row][code(i)] - q[right_row][code(i)] for a valid k-mer, 0 otherwise
    P(p) = sum_{lo <= i < p} d(i),  p = lo .. hi
    position = the p of the largest P; ties to the smallest |p - x|, then to the smallest p
    gain = P(position) - P(x), left_evidence = P(position) - P(lo), right_evidence = P(position) - P(hi)
    support = the valid k-mers starting in [lo, hi)
"""
import numpy as np


def codes(sequence, k, symbols="ATGC"):
    """code(i) for every i of the sequence, -1 for a k-mer that is not valid."""
    digit = {c: d for d, c in enumerate(symbols)}
    L = len(sequence)
    out = []
    for i in range(L):
        code = -1
        if i + k <= L:
            code = 0
            for c in sequence[i:i + k]:
                if c not in digit:
                    code = -1
                    break
                code = code * 4 + digit[c]
        out.append(code)
    return out


def refine_one(code, q_left, q_right, lo, x, hi):
    """(position, gain, left_evidence, right_evidence, support) of one boundary; ``code`` = ``codes`` of its sequence, the rows
    lists of Python ints."""
    assert 0 <= lo <= x <= hi <= len(code)
    P, support = 0, 0
    best_P, best_p = 0, lo                                  # the candidate p = lo: P(lo) = 0
    P_x = 0 if x == lo else None
    for i in range(lo, hi):
        if code[i] >= 0:
            P += q_left[code[i]] - q_right[code[i]]
            support += 1
        p = i + 1
        if P > best_P or (P == best_P and (abs(p - x) < abs(best_p - x) or (abs(p - x) == abs(best_p - x) and p < best_p))):
            best_P, best_p = P, p
        if p == x:
            P_x = P
    return best_p, best_P - P_x, best_P, best_P - P, support


def refine(sequences, k, q, seq, lo, x, hi, left_row, right_row, symbols="ATGC"):
    """(position (B,), evidence (B, 3), support (B,)) int64 arrays of the statement; q (n_rows, D) integers."""
    rows = [[int(v) for v in row] for row in np.asarray(q)]
    cache = {}
    B = len(seq)
    position, evidence, support = np.zeros(B, dtype=np.int64), np.zeros((B, 3), dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        s = int(seq[b])
        if s not in cache:
            cache[s] = codes(sequences[s], k, symbols)
        p, g, le, re, n = refine_one(cache[s], rows[int(left_row[b])], rows[int(right_row[b])], int(lo[b]), int(x[b]), int(hi[b]))
        position[b], support[b] = p, n
        evidence[b] = (g, le, re)
    return position, evidence, support


def boundary_plan(state, owner, start, window, step, span=None):
    """``compose.boundary_plan`` as a loop: the lists (record, x, lo, hi, left_state, right_state, first_window) with one entry
    per pair of adjacent runs of one record."""
    state, owner, start = [int(v) for v in state], [int(v) for v in owner], [int(v) for v in start]
    window, step = int(window), int(step)
    span = window if span is None else int(span)
    runs = []
    for t in range(len(state)):
        if runs and owner[runs[-1][1]] == owner[t] and state[runs[-1][1]] == state[t]:
            runs[-1][1] = t
        else:
            runs.append([t, t])
    out = [[] for _ in range(7)]
    for (a0, a1), (b0, b1) in zip(runs[:-1], runs[1:]):
        if owner[a0] != owner[b0]:
            continue
        x = (start[a1] + window + start[b0]) // 2
        left_mid = (start[a0] + start[a1] + window) // 2
        right_mid = (start[b0] + start[b1] + window) // 2
        lo = min(x, max(x - span, left_mid + 1))
        hi = max(x, min(x + span, right_mid))
        for col, v in zip(out, (owner[a0], x, lo, hi, state[a0], state[b0], b0)):
            col.append(v)
    return out


def read_fasta(path):
    """(ids, sequences) of a small FASTA file."""
    ids, seqs = [], []
    for line in open(path):
        if line.startswith(">"):
            ids.append(line[1:].split()[0])
            seqs.append("")
        else:
            seqs[-1] += line.strip()
    return ids, seqs
