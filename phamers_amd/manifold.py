"""
manifold.py -- the embedding behind phamer_scorer.do_tsne (scripts/phamer.py:337-366): scikit-learn's PCA and TSNE on the
device, float64, bit-identical from run to run.

    PCA(n_components).fit_transform(X)            sklearn.decomposition.PCA(svd_solver='full')  -> GPU covariance (fp64 MFMA) +
                                                                                                    host eigh (D x D) + GPU projection
    TSNE(...).fit_transform(X)                    sklearn.manifold.TSNE(method='barnes_hut')    -> GPU, every stage below
    neighbor_affinities(Z, perplexity)            kneighbors_graph + _binary_search_perplexity  -> GPU (distance rows + radix select;
                                                                                                    one thread per row's search)
    Affinities.joint()                            _joint_probabilities_nn's P + P.T, / sum      -> host C, reverse adjacency, O(n k)
    kl_gradient(Y, affinities, exaggeration)      _kl_divergence (objective and gradient)       -> GPU, repulsion over ALL pairs
    descend(Y0, affinities, n_steps, ...)         _gradient_descent, exactly n_steps updates    -> GPU, one C call

Differences from scikit-learn 1.7, all deliberate:
  * the repulsive term of the gradient is summed exactly over all pairs (the angle -> 0 limit of Barnes-Hut) in float64;
    ``angle`` is accepted and not used.  The embedding is therefore not scikit-learn's coordinate for coordinate (its own
    depends on thread count and float32 tree order); it is held to scikit-learn's quality (KL, trustworthiness) instead;
  * the perplexity search runs on float64 squared direct-difference distances (scikit-learn: the square of a float64
    distance, cast to float32); the embedding, gradient and update are float64 (scikit-learn: float32 embedding);
  * neighbours are ordered by (distance, index), ties between identical distances decided by the index;
  * init='pca' takes the first two components of the exact PCA above (scikit-learn: a randomized solver seeded by
    ``random_state``), scaled by 1e-4 / std(first component) in float64.

The D x D symmetric eigenproblem of PCA runs on the host (numpy.linalg.eigh): it does not depend on n, as the k-means
seeding does not; at D = 256 it takes 12 ms, at D = 4096 21 s on one core of the development host.
"""
import ctypes

import numpy as np

from . import _lib

MACHINE_EPSILON = np.finfo(np.double).eps
_EXPLORATION_MAX_ITER = 250      # TSNE._EXPLORATION_MAX_ITER
_N_ITER_CHECK = 50               # TSNE._N_ITER_CHECK
K_MAX = 4096                     # neighbours per row the device selection sorts (perplexity <= 1365)


def _check_finite(X):
    """scikit-learn's check_array messages for NaN / infinite input."""
    if np.isnan(X).any():
        raise ValueError("Input contains NaN.")
    if np.isinf(X).any():
        raise ValueError("Input contains infinity or a value too large for dtype('float64').")


def _matrix(X, name="X"):
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("%s must be 2-D, got shape %s" % (name, X.shape))
    _check_finite(X)
    return X


class PCA(object):
    """sklearn.decomposition.PCA(n_components, svd_solver='full'): ``fit_transform``, ``transform``, ``components_``,
    ``mean_``, ``explained_variance_``.  The sign of each component is scikit-learn's svd_flip(u_based_decision=False): its
    largest-magnitude entry is positive."""

    def __init__(self, n_components):
        self.n_components = int(n_components)
        self.components_ = self.mean_ = self.explained_variance_ = None

    def fit(self, X):
        X = _matrix(X)
        n, D = X.shape
        c = self.n_components
        if not 1 <= c <= min(n, D):
            raise ValueError("n_components=%r must be between 1 and min(n_samples, n_features)=%r with svd_solver='full'"
                             % (c, min(n, D)))
        if n < 2:
            raise ValueError("PCA needs at least 2 samples")
        ctx = _lib.get_context()
        mean = np.empty(D, dtype=np.float64)
        cov = np.empty((D, D), dtype=np.float64)
        _lib.check(ctx.lib.phk_pca_covariance(ctx.handle, _lib.ptr(X), n, D, _lib.ptr(mean), _lib.ptr(cov)))
        w, v = np.linalg.eigh(cov)               # ascending
        order = np.argsort(-w, kind="stable")[:c]
        comps = np.ascontiguousarray(v[:, order].T)
        # svd_flip(u_based_decision=False): the largest-|.| entry of each row positive
        big = np.argmax(np.abs(comps), axis=1)
        comps *= np.sign(comps[np.arange(c), big])[:, None]
        self.mean_, self.components_ = mean, comps
        self.explained_variance_ = np.maximum(w[order], 0.0)
        return self

    def transform(self, X):
        X = _matrix(X)
        if self.components_ is None:
            raise ValueError("This PCA instance is not fitted yet.")
        n, D = X.shape
        if D != self.mean_.shape[0]:
            raise ValueError("X has %d features, but PCA is expecting %d features as input." % (D, self.mean_.shape[0]))
        c = self.components_.shape[0]
        out = np.empty((n, c), dtype=np.float64)
        ctx = _lib.get_context()
        _lib.check(ctx.lib.phk_pca_project(ctx.handle, _lib.ptr(X), n, D, _lib.ptr(self.mean_), _lib.ptr(self.components_), c,
                                           _lib.ptr(out)))
        return out

    def fit_transform(self, X):
        X = _matrix(X)
        return self.fit(X).transform(X)


class Affinities(object):
    """What neighbor_affinities returns; unpacks as (indices, sqdistances, conditional, beta).  ``joint()`` is the
    symmetric P = (P + P.T) / sum as CSR arrays (indptr int64, indices int32, values float64), built once."""

    def __init__(self, indices, sqdistances, conditional, beta):
        self.indices, self.sqdistances, self.conditional, self.beta = indices, sqdistances, conditional, beta
        self._joint = None

    def __iter__(self):
        return iter((self.indices, self.sqdistances, self.conditional, self.beta))

    def joint(self):
        if self._joint is None:
            self._joint = symmetrize(self.indices, self.conditional)
        return self._joint


def n_neighbors_for(n_samples, perplexity):
    """TSNE._fit: min(n_samples - 1, int(3 * perplexity + 1))."""
    return min(int(n_samples) - 1, int(3.0 * perplexity + 1))


def neighbors(Z, k):
    """The k nearest other rows of every row of Z: (indices (n, k) int32, squared distances (n, k) float64), ordered by
    (distance, index); distances are float64 direct differences (phk_tsne_neighbors)."""
    Z = _matrix(Z, "Z")
    n, d = Z.shape
    k = int(k)
    if not 1 <= k <= min(n - 1, K_MAX):
        raise ValueError("k=%d neighbours: must be between 1 and min(n_samples - 1, %d)" % (k, K_MAX))
    idx = np.empty((n, k), dtype=np.int32)
    d2 = np.empty((n, k), dtype=np.float64)
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_tsne_neighbors(ctx.handle, _lib.ptr(Z), n, d, k, _lib.ptr(idx), _lib.ptr(d2)))
    return idx, d2


def conditional_affinities(sqdistances, perplexity):
    """scikit-learn's _binary_search_perplexity on float64 squared distances (n, k): (P (n, k), beta (n,)).  The target
    entropy is log(float32(perplexity)), as in scikit-learn, whose argument is a C float."""
    d2 = np.ascontiguousarray(sqdistances, dtype=np.float64)
    n, k = d2.shape
    P = np.empty((n, k), dtype=np.float64)
    beta = np.empty(n, dtype=np.float64)
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_tsne_affinities(ctx.handle, _lib.ptr(d2), n, k, float(np.float32(perplexity)), _lib.ptr(P),
                                           _lib.ptr(beta)))
    return P, beta


def symmetrize(indices, conditional):
    """(P + P.T) / sum over the union of the directed edges: CSR (indptr, indices, values), columns ascending in a row."""
    idx = np.ascontiguousarray(indices, dtype=np.int32)
    P = np.ascontiguousarray(conditional, dtype=np.float64)
    n, k = idx.shape
    indptr = np.empty(n + 1, dtype=np.int64)
    cols = np.empty(2 * n * k, dtype=np.int32)
    vals = np.empty(2 * n * k, dtype=np.float64)
    nnz = ctypes.c_uint64()
    _lib.check(_lib.load().phk_tsne_symmetrize(_lib.ptr(idx), _lib.ptr(P), n, k, _lib.ptr(indptr), _lib.ptr(cols), _lib.ptr(vals),
                                               ctypes.byref(nnz)))
    return indptr, cols[:nnz.value].copy(), vals[:nnz.value].copy()


def neighbor_affinities(Z, perplexity):
    """Stages 2 and 3 of TSNE._fit for the rows of Z: an Affinities of neighbour indices (n, k), squared distances,
    conditional P and beta, k = min(n - 1, int(3 * perplexity + 1))."""
    Z = _matrix(Z, "Z")
    if perplexity >= Z.shape[0]:
        raise ValueError("perplexity must be less than n_samples")
    idx, d2 = neighbors(Z, n_neighbors_for(Z.shape[0], perplexity))
    P, beta = conditional_affinities(d2, perplexity)
    return Affinities(idx, d2, P, beta)


def _csr(affinities):
    indptr, cols, vals = affinities.joint() if isinstance(affinities, Affinities) else affinities
    return (np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(cols, dtype=np.int32),
            np.ascontiguousarray(vals, dtype=np.float64))


def _embedding(Y, n):
    Y = np.array(Y, dtype=np.float64, order="C")
    if Y.shape != (n, 2):
        raise ValueError("the embedding must be (%d, 2), got %s" % (n, Y.shape))
    _check_finite(Y)
    return Y


def kl_gradient(Y, affinities, exaggeration=1.0):
    """(KL, grad (n, 2)) of the embedding Y for the symmetric affinities times ``exaggeration``: the objective over the
    sparse P with the exact Q, the repulsive term over all pairs (phk_tsne_gradient)."""
    indptr, cols, vals = _csr(affinities)
    n = indptr.shape[0] - 1
    Y = _embedding(Y, n)
    grad = np.empty((n, 2), dtype=np.float64)
    kl = ctypes.c_double()
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_tsne_gradient(ctx.handle, _lib.ptr(Y), n, _lib.ptr(indptr), _lib.ptr(cols), _lib.ptr(vals),
                                         float(exaggeration), ctypes.byref(kl), _lib.ptr(grad)))
    return kl.value, grad


def descend(Y0, affinities, n_steps, exaggeration=1.0, momentum=0.8, learning_rate=200.0, min_gain=0.01):
    """Y after exactly ``n_steps`` updates of scikit-learn's _gradient_descent from Y0 (update 0, gains 1), in one call."""
    indptr, cols, vals = _csr(affinities)
    n = indptr.shape[0] - 1
    Y = _embedding(Y0, n)
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_tsne_descend(ctx.handle, _lib.ptr(Y), n, _lib.ptr(indptr), _lib.ptr(cols), _lib.ptr(vals),
                                        float(exaggeration), float(momentum), float(learning_rate), float(min_gain), int(n_steps),
                                        None))
    return Y


class TSNE(object):
    """sklearn.manifold.TSNE for n_components=2, metric='euclidean', method='barnes_hut' with the repulsion summed exactly
    (see the module docstring): ``fit_transform``, ``embedding_``, ``kl_divergence_``, ``n_iter_``, ``learning_rate_``.
    ``angle`` is accepted and not used."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, metric='euclidean', init='pca', verbose=0, random_state=None,
                 method='barnes_hut', angle=0.5):
        self.n_components, self.perplexity, self.early_exaggeration = n_components, perplexity, early_exaggeration
        self.learning_rate, self.max_iter, self.n_iter_without_progress = learning_rate, max_iter, n_iter_without_progress
        self.min_grad_norm, self.metric, self.init, self.verbose = min_grad_norm, metric, init, verbose
        self.random_state, self.method, self.angle = random_state, method, angle
        self.embedding_ = self.kl_divergence_ = self.n_iter_ = self.learning_rate_ = None

    def _initial(self, X):
        n = X.shape[0]
        if isinstance(self.init, np.ndarray):
            return _embedding(self.init, n)
        if self.init == 'pca':
            Y = PCA(2).fit_transform(X)
            return Y / np.std(Y[:, 0]) * 1e-4
        if self.init == 'random':
            rs = self.random_state if isinstance(self.random_state, np.random.RandomState) else np.random.RandomState(self.random_state)
            return 1e-4 * rs.standard_normal(size=(n, 2))
        raise ValueError("init must be 'pca', 'random' or an array, got %r" % (self.init,))

    def fit_transform(self, X):
        if self.n_components != 2:
            raise NotImplementedError("TSNE on the device embeds into 2 dimensions (n_components=%r)" % (self.n_components,))
        if self.metric != 'euclidean':
            raise NotImplementedError("TSNE on the device: metric='euclidean' only (got %r)" % (self.metric,))
        if self.method != 'barnes_hut':
            raise NotImplementedError("TSNE on the device keeps the sparse neighbour affinities of method='barnes_hut'; "
                                      "method=%r (a dense P) is not implemented" % (self.method,))
        if self.max_iter < _EXPLORATION_MAX_ITER:
            raise ValueError("max_iter must be at least %d" % _EXPLORATION_MAX_ITER)
        X = _matrix(X)
        n = X.shape[0]
        if self.perplexity >= n:
            raise ValueError("perplexity must be less than n_samples")
        if self.learning_rate == 'auto':
            self.learning_rate_ = max(n / self.early_exaggeration / 4, 50)
        else:
            self.learning_rate_ = self.learning_rate
        indptr, cols, vals = neighbor_affinities(X, self.perplexity).joint()
        Y = self._initial(X)
        kl, it = ctypes.c_double(), ctypes.c_uint64()
        ctx = _lib.get_context()
        _lib.check(ctx.lib.phk_tsne_fit(ctx.handle, _lib.ptr(Y), n, _lib.ptr(indptr), _lib.ptr(cols), _lib.ptr(vals),
                                        float(self.early_exaggeration), float(self.learning_rate_), int(self.max_iter),
                                        int(self.n_iter_without_progress), float(self.min_grad_norm), ctypes.byref(kl),
                                        ctypes.byref(it)))
        self.embedding_, self.kl_divergence_, self.n_iter_ = Y, kl.value, int(it.value)
        if self.verbose:
            print("[t-SNE] KL divergence after %d iterations: %f" % (self.n_iter_ + 1, self.kl_divergence_))
        return Y

    def fit(self, X):
        self.fit_transform(X)
        return self
