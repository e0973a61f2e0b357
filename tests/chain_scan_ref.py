"""The statement of the tile scan of the S-state chain (csrc/chain.hip) and the bounds derived for
it.  The model, the exact statements and the bounds of the per-record route are tests/compose_ref.py's; nothing of them is
restated here.

The route.  A record of n windows is cut into K = ceil(n / TILE) tiles of TILE consecutive windows from its own start.  With
e_t = exp(d[t]) and q[t] as compose_ref states them, a step t that is not the record's first has the sum-product matrix
M_t = A diag(e_t) and the max-plus matrix Q_t[i][j] = qlogA[i][j] + q[t][j].  A tile's F (float64, rescaled by powers of two
with the exponent kept as an integer) and V (integers) are the ordered products of its steps; the record's first tile starts
from pi and is a vector.  The carry takes alpha (left to right), beta (right to left) and delta (left to right) through the
tiles in tile order; a tile then runs the per-step recurrences from the vectors that enter it; a record's xi is the sum of
its tiles' xi in tile order.

``tile_forward_backward`` states that route in float64 NumPy, ``tile_viterbi`` in Python ints.  Integer max-plus is
associative, so ``tile_viterbi`` must give compose_ref.viterbi's path and score exactly.

Bounds (u = 2^-53).  Every float quantity is a sum of products of positive numbers, so to first order its relative error is
u times the roundings on the deepest path through it.  The factors of alpha_t beta_t are the n steps of the record, each of
them once, whichever route forms them; inside a tile's F a step costs what it costs in compose_ref's count (S products, S - 1
additions, the product with e, e's own error).  What the route adds is the carry: alpha entering a tile has passed one
vector-matrix product per tile before it, beta leaving a tile one per tile after it, and such a product costs S products and
S - 1 additions on a path, 2 S - 1 <= 2 S + 2 roundings (the power-of-two rescalings are exact).  A posterior's numerator and
its denominator each carry at most K such products between alpha and beta together, hence

    B_scan(n, S) = B(n, S) + 2 K (2 S + 2) u,      K = ceil(n / TILE)

xi of a record: a term passes through at most TILE - 1 additions inside its tile and K - 1 in the fold, no more than the
n of compose_ref's count, so (B_scan + n u) exact + n FLOOR as there.  T and N_s add the same terms as there.  The evidence
takes alpha through every tile: K (2 S + 2) u more; its sum of the n maxima is a sum in another order, which the
n u sum|M| term covers whatever the order.
"""
import numpy as np

from tests import compose_ref as cref
from tests.segment_ref import FLOOR, LD, U

TILE = 64


def n_tiles(n, tile=TILE):
    return -(-int(n) // int(tile))


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def carry_error(n, S, tile=TILE):
    return n_tiles(n, tile) * (2.0 * S + 2.0) * U


def scan_posterior_bound(n, S, tile=TILE):
    """B_scan(n, S) for a record of n windows."""
    return cref.posterior_bound(n, S) + 2.0 * carry_error(n, S, tile)


def scan_evidence_bound(M, S, log_evidence, tile=TILE):
    """For one record with row maxima ``M`` (n,)."""
    return cref.evidence_bound(M, S, log_evidence) + carry_error(len(M), S, tile)


def check_posterior(got, exact, n_longest, S, what="", extra=0.0, tile=TILE):
    """|got - exact| <= (B_scan + extra) exact + FLOOR; returns the worst error / bound."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=LD)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(LD) - exact)
    bound = LD(scan_posterior_bound(n_longest, S, tile) + extra) * exact + LD(FLOOR)
    worst = float((err / bound).max()) if err.size else 0.0
    assert not (err > bound).any(), "%s: %d posteriors outside B_scan(n, S); worst error / bound %.3g" % (
        what, int((err > bound).sum()), worst)
    return worst


def check_sums(got, exact, n_longest, S, terms, floor_terms, what="", tile=TILE):
    """A sum of ``terms`` positive terms each inside B_scan: (B_scan + (terms + 2) u) exact + floor_terms FLOOR."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=LD)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(LD) - exact)
    bound = LD(scan_posterior_bound(n_longest, S, tile) + (terms + 2.0) * U) * exact + LD(FLOOR) * LD(floor_terms)
    worst = float((err / np.maximum(bound, LD(1e-4000))).max()) if err.size else 0.0
    assert not (err > bound).any(), "%s: worst error / bound %.3g" % (what, worst)
    return worst


def check_evidence(got, exact, M, S, what="", tile=TILE):
    err = abs(LD(float(got)) - LD(exact))
    bound = scan_evidence_bound(M, S, exact, tile)
    assert np.isfinite(float(got)) and err <= bound, "%s: evidence error %.3g, bound %.3g" % (what, float(err), bound)
    return float(err) / bound


# ---- the float64 statement ---------------------------------------------------------------------------------------------------
def _scale2(v):
    """(v / 2^e, e) with e the exponent of v's largest entry: exact."""
    e = int(np.frexp(v.max())[1])
    return np.ldexp(v, -e), e


def _bounds(n, tile):
    return [(a, min(a + tile, n)) for a in range(0, n, tile)]


def tile_products(e, M, A, pi, tile=TILE):
    """Per tile: F (S, S) rescaled, its exponent, the sum of the tile's M.  The first tile's rows are all the vector from pi."""
    S = len(pi)
    out = []
    for k, (a, b) in enumerate(_bounds(len(e), tile)):
        f = np.tile(pi * e[a], (S, 1)) if k == 0 else A * e[a][None, :]
        f, fe = _scale2(f)
        sm = M[a]
        for w in range(a + 1, b):
            f, x = _scale2((f @ A) * e[w][None, :])
            fe += x
            sm = sm + M[w]
        out.append((f, fe, sm))
    return out


def tile_forward_backward(E, trans, init, tile=TILE):
    """One record by the tile route in float64: (gamma (n, S), xi (S, S), gamma_0 (S,), log evidence); zeros for n = 0."""
    E = np.asarray(E, dtype=np.float64)
    n, S = E.shape
    A, pi = np.asarray(trans, dtype=np.float64), np.asarray(init, dtype=np.float64)
    if n == 0:
        return np.zeros((0, S)), np.zeros((S, S)), np.zeros(S), 0.0
    with np.errstate(under='ignore'):
        e = np.exp(cref.relative(E))
        M = E.max(axis=1)
        tiles = tile_products(e, M, A, pi, tile)
        K = len(tiles)
        # the carry
        al, ex, sm = tiles[0][0][0].copy(), tiles[0][1], tiles[0][2]
        enter = [None]
        for k in range(1, K):
            enter.append(al)
            al, x = _scale2(al @ tiles[k][0])
            ex += tiles[k][1] + x
            sm = sm + tiles[k][2]
        m, e2 = np.frexp(al.sum())
        evidence = ((ex + int(e2)) * np.log(2.0) + np.log(m)) + sm
        leave, be = [None] * K, np.ones(S)
        for k in range(K - 1, -1, -1):
            leave[k] = be
            if k:
                be = _scale2(tiles[k][0] @ be)[0]
        # the walk
        gamma, xi, g0 = np.zeros((n, S)), np.zeros((S, S)), None
        for k, (a, b) in enumerate(_bounds(n, tile)):
            B = np.zeros((b - a, S))
            bv = leave[k]
            for w in range(b - 1, a - 1, -1):
                B[w - a] = bv
                if w > a:
                    bv = _scale2(A @ (e[w] * bv))[0]
            x = np.zeros((S, S))
            w = a
            if k == 0:
                p = pi * (e[a] * B[0])
                gamma[a] = g0 = p / p.sum()
                al = _scale2(pi * e[a])[0]
                w = a + 1
            else:
                al = enter[k]
            for w in range(w, b):
                pr = al[:, None] * A
                wv = pr * (e[w] * B[w - a])[None, :]
                col = wv.sum(axis=0)
                inv = 1.0 / col.sum()
                x += wv * inv
                gamma[w] = col * inv
                al = _scale2(pr.sum(axis=0) * e[w])[0]
            xi = xi + x                       # the fold: in tile order
    return gamma, xi, g0, float(evidence)


# ---- the integer statement -----------------------------------------------------------------------------------------------------
def tile_viterbi(q, qlog_trans, qlog_init, tile=TILE):
    """(states (n,) uint8, score int) of one record's integer emissions ``q`` by the tile route: tile products, the carry of
    delta, the walk inside every tile with its map, the ends through the maps, the fill."""
    n = len(q)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), 0
    S = len(q[0])
    qa = [[int(qlog_trans[i][j]) for j in range(S)] for i in range(S)]
    qp = [int(v) for v in qlog_init]
    bounds = _bounds(n, tile)
    # tile products
    V = []
    for k, (a, b) in enumerate(bounds):
        v = [[(qp[j] if k == 0 else qa[i][j]) + q[a][j] for j in range(S)] for i in range(S)]
        for w in range(a + 1, b):
            v = [[max(v[i][m] + qa[m][j] for m in range(S)) + q[w][j] for j in range(S)] for i in range(S)]
        V.append(v)
    # the carry
    d, enter = list(V[0][0]), [None]
    for k in range(1, len(V)):
        enter.append(d)
        d = [max(d[i] + V[k][i][j] for i in range(S)) for j in range(S)]
    s = 0
    for j in range(1, S):
        if d[j] > d[s]:
            s = j
    score = d[s]
    # the walk: backpointers of every step but the record's first, and the tile's map
    back, maps = [None] * n, []
    for k, (a, b) in enumerate(bounds):
        d = [qp[j] + q[a][j] for j in range(S)] if k == 0 else enter[k]
        org = list(range(S))
        for w in range(a + 1 if k == 0 else a, b):
            nd, bp = [], []
            for j in range(S):
                best, arg = d[0] + qa[0][j], 0
                for i in range(1, S):
                    c = d[i] + qa[i][j]
                    if c > best:
                        best, arg = c, i
                nd.append(best + q[w][j])
                bp.append(arg)
            d, back[w] = nd, bp
            org = [org[m] for m in bp]
        maps.append(org)
    # the ends, then the fill
    ends = [0] * len(bounds)
    for k in range(len(bounds) - 1, -1, -1):
        ends[k] = s
        s = maps[k][s]
    states = np.empty(n, dtype=np.uint8)
    for k, (a, b) in enumerate(bounds):
        s = ends[k]
        for w in range(b - 1, a - 1, -1):
            states[w] = s
            if back[w] is not None:
                s = back[w][s]
    return states, score
