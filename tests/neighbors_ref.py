"""numpy restatement of the neighbour rules of include/loco_asr.h ("embedding neighbours") -- the checker, never the product.

No reference program exists for these (sentence-transformers and scikit-learn are not available): the rules are the project's own,
restated here in float64 with the plainest numpy there is, and the device code is pinned against this.

* scores in float64: dot ``q.k``; cosine ``((q.k) * inv_q) * inv_k`` with ``inv = 1 / max(sqrt(norm2), 1e-12)``; l2
  ``(2 (q.k) - norm2_k) - norm2_q``;
* selection by ``np.lexsort((index, -score))`` over the candidates: not NaN, not the query's ``exclude`` entry;
* group mean in float64; Lloyd's algorithm with the same rules, which also returns every round's smallest best-to-second margin.
"""
import numpy as np

D = 768


def norm2(x):
    x = np.asarray(x, np.float64)
    return (x * x).sum(axis=1)


def scores(Q, K, metric):
    Q, K = np.asarray(Q, np.float64), np.asarray(K, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dot = Q @ K.T
        if metric == "dot":
            return dot
        if metric == "cosine":
            inv_q = 1.0 / np.maximum(np.sqrt(norm2(Q)), 1e-12)
            inv_k = 1.0 / np.maximum(np.sqrt(norm2(K)), 1e-12)
            return (dot * inv_q[:, None]) * inv_k[None, :]
        if metric == "l2":
            return (2.0 * dot - norm2(K)[None, :]) - norm2(Q)[:, None]
    raise ValueError(metric)


def select(S, k, exclude=None):
    """(values f64 [M, k], indices i32 [M, k]) of a score matrix: best first, ties to the lower index, (-inf, -1) tails."""
    S = np.asarray(S, np.float64)
    M, N = S.shape
    values = np.full((M, k), -np.inf)
    indices = np.full((M, k), -1, np.int32)
    for i in range(M):
        cand = ~np.isnan(S[i])
        if exclude is not None and 0 <= int(exclude[i]) < N:
            cand[int(exclude[i])] = False
        idx = np.flatnonzero(cand)
        order = idx[np.lexsort((idx, -S[i, idx]))][:k]
        values[i, :order.size] = S[i, order]
        indices[i, :order.size] = order
    return values, indices


def topk(Q, K, k, metric, exclude=None):
    return select(scores(Q, K, metric), k, exclude)


def brute_force(S, k, exclude=None):
    """The same selection with Python's sort over (−score, index) tuples: what ``select`` is checked against."""
    S = np.asarray(S, np.float64)
    out_v, out_i = [], []
    for i in range(S.shape[0]):
        rows = [(-S[i, j], j) for j in range(S.shape[1]) if S[i, j] == S[i, j] and not (exclude is not None and exclude[i] == j)]
        rows.sort()
        rows = rows[:k]
        out_v.append([-v for v, _ in rows] + [-np.inf] * (k - len(rows)))
        out_i.append([j for _, j in rows] + [-1] * (k - len(rows)))
    return np.asarray(out_v, np.float64).reshape(S.shape[0], k), np.asarray(out_i, np.int32).reshape(S.shape[0], k)


def group_mean(rows, offsets, index=None, out=None):
    """(out f32 [G, 768], count): float64 mean of each group's rows, rounded to float32; an empty group keeps ``out``'s row."""
    rows = np.asarray(rows, np.float64)
    G = len(offsets) - 1
    out = np.zeros((G, rows.shape[1]), np.float32) if out is None else np.array(out, np.float32)
    count = np.zeros(G, np.int32)
    for g in range(G):
        a, b = int(offsets[g]), int(offsets[g + 1])
        count[g] = b - a
        if b > a:
            src = np.arange(a, b) if index is None else np.asarray(index)[a:b]
            out[g] = rows[src].mean(axis=0).astype(np.float32)
    return out, count


def recall_at_k(indices, partner, ks):
    indices, partner = np.asarray(indices), np.asarray(partner)
    return {int(k): float(np.mean([(partner[i] in indices[i, :k]) for i in range(indices.shape[0])])) for k in ks}


def vote(neighbour_labels, n_classes):
    """The most frequent class of each row (-1 = no neighbour), ties to the lowest class id."""
    out = []
    for row in np.asarray(neighbour_labels):
        votes = np.zeros(n_classes, np.int64)
        for c in row:
            if c >= 0:
                votes[c] += 1
        out.append(int(np.flatnonzero(votes == votes.max())[0]))
    return np.asarray(out, np.int64)


def knn_classify(train, labels, queries, k, n_classes, exclude=None, metric="cosine"):
    _, idx = topk(queries, train, k, metric, exclude)
    labels = np.asarray(labels)
    return vote(np.where(idx >= 0, labels[np.maximum(idx, 0)], -1), n_classes)


def pairs_from_topk(values, indices, top_k):
    """Unordered pairs (i < j) of the rows' entries, each once with the score of the row of its lower index where that row lists it,
    by (score desc, i asc, j asc)."""
    values, indices = np.asarray(values), np.asarray(indices)
    found = {}
    for r in range(indices.shape[0]):
        for v, c in zip(values[r], indices[r]):
            c = int(c)
            if c < 0 or c == r:
                continue
            key = (min(r, c), max(r, c))
            lower = r == key[0]
            if key not in found or (lower and not found[key][1]):
                found[key] = (v, lower)
    rows = sorted(((-float(v), i, j) for (i, j), (v, _) in found.items()))[:top_k]
    return [(i, j) for _, i, j in rows], [-v for v, _, _ in rows]


def cluster_purity(labels, classes):
    labels, classes = np.asarray(labels), np.asarray(classes)
    right = 0
    for c in np.unique(labels):
        right += np.bincount(classes[labels == c]).max()
    return right / labels.shape[0]


def inertia_of(top1_values):
    """The sum of the negated top-1 values in double, in point order."""
    total = 0.0
    for v in np.asarray(top1_values, np.float64):
        total += -v
    return total


def kmeans(X, init, iters):
    """Lloyd's algorithm by the rules of neighbors.kmeans.  Returns a list of rounds, each a dict of ``labels`` (i32), ``centers`` (the
    f32 centres the labels were assigned against), ``inertia`` (float64 scores) and ``margin`` (the smallest best-to-second score gap;
    inf with one centre), and the final centres."""
    X = np.asarray(X, np.float32)
    centers = X[np.asarray(init)].copy()
    C = centers.shape[0]
    rounds, prev = [], None
    for rnd in range(iters):
        vals, idx = topk(X, centers, min(2, C), "l2")
        labels = idx[:, 0].astype(np.int32)
        margin = float((vals[:, 0] - vals[:, 1]).min()) if C > 1 else float("inf")
        rounds.append({"labels": labels, "centers": centers.copy(), "inertia": inertia_of(vals[:, 0]), "margin": margin})
        if prev is not None and np.array_equal(labels, prev):
            break
        if rnd + 1 == iters:
            break
        order = np.argsort(labels, kind="stable")
        offsets = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=C))])
        centers, _ = group_mean(X, offsets, order, out=centers)
        prev = labels
    return rounds, centers


# ---- the inputs the GPU tests and the CPU preconditions share -------------------------------------------------------------------------
def kmeans_input():
    """(X f32 [640, 768], init [8], planted labels [640]): Generator(Philox(20250102)), 8 centres N(0, 1), 80 points per centre with
    noise 0.3, one permutation of the points, init = the first row of each planted cluster."""
    g = np.random.Generator(np.random.Philox(20250102))
    centres = g.standard_normal((8, D))
    pts = np.repeat(centres, 80, axis=0) + 0.3 * g.standard_normal((640, D))
    planted = np.repeat(np.arange(8), 80)
    perm = g.permutation(640)
    X = pts[perm].astype(np.float32)
    planted = planted[perm]
    init = np.asarray([int(np.flatnonzero(planted == c)[0]) for c in range(8)])
    return X, init, planted


def kmeans_margin_bound(X, centers):
    """4 * 768 * 2^-24 * max(|x|^2, |c|^2): what an fp32 l2 score can be off by, with room."""
    return 4.0 * D * 2.0 ** -24 * max(norm2(X).max(), norm2(centers).max())


def cosine_input():
    """(Q f32 [300, 768], K f32 [2049, 768]): z W / sqrt(6) + 0.3 noise with a 6-dimensional latent, Philox seed 20250101."""
    g = np.random.Generator(np.random.Philox(20250101))
    W = g.standard_normal((6, D))
    Q = g.standard_normal((300, 6)) @ W / np.sqrt(6.0) + 0.3 * g.standard_normal((300, D))
    K = g.standard_normal((2049, 6)) @ W / np.sqrt(6.0) + 0.3 * g.standard_normal((2049, D))
    return Q.astype(np.float32), K.astype(np.float32)


def integer_input(M=300, N=2049, seed=20250103):
    """(Q, K) with entries from {-2 .. 2}: every dot product and squared norm is an integer below 2^24, exact in fp32 in any order."""
    g = np.random.Generator(np.random.Philox(seed))
    return g.integers(-2, 3, (M, D)).astype(np.float32), g.integers(-2, 3, (N, D)).astype(np.float32)
