"""Embedding neighbours on the device: fused top-k, recall, kNN voting, pair mining and k-means (csrc/neighbors.hip).

The reference's notebooks mean-pool the encoder output, form ``util.cos_sim`` matrices, mine the best pairs, run ``KMeans`` and look at
how utterances group by intent.  Here the N x N matrix is never formed: ``topk`` walks the exact-fp32 MFMA product in 128 x 128 tiles
and every query keeps a sorted list of its k best keys (``loco_op_topk``); everything else in this module stands on it.

The rules (include/loco_asr.h, "embedding neighbours"):

* ``dot``: ``s = q.k``; ``cosine``: ``s = ((q.k) * inv_q) * inv_k`` with ``inv = 1 / max(sqrt(norm2), 1e-12)``
  (``torch.nn.functional.normalize``'s eps, which ``util.cos_sim`` uses; a zero vector scores 0); ``l2``:
  ``s = (2 (q.k) - norm2_k) - norm2_q``, the negated squared distance, so larger always means closer.
* Results are best first, ties towards the LOWER key index.  A NaN score is not a candidate, nor is a query's ``exclude`` entry.
  Where fewer than k candidates exist the remaining slots hold index -1 and value -inf.
* A query's k results are a function of that query's 768 values, its ``exclude`` entry and the keys alone, bit for bit: not of the
  number of queries, of the query's row or of the slab it fell into.

Nothing here is validated against sentence-transformers or scikit-learn (neither is available where this project is built): parity is
pinned against numpy restatements of the rules above (tests/neighbors_ref.py).  There is no CPU path: the products run in
``loco_op_topk`` or not at all.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _lib

D = 768
MAX_K = 16  # LOCO_TOPK_MAX_K (checked against the library on first use)
METRICS = {"dot": 0, "cosine": 1, "l2": 2}
SCRATCH_CAP = 1 << 30  # bytes of (query, chunk) records one launch may use: more queries are split into slabs, which changes no result
_CHUNK = 1024


@dataclass
class TopK:
    """``values`` f32 [M, k] and ``indices`` i32 [M, k] on the device, best first; (-inf, -1) where fewer than k candidates exist."""
    values: torch.Tensor
    indices: torch.Tensor


@dataclass
class KMeansResult:
    """``labels`` i32 [N] and ``centers`` f32 [C, 768] on the device; ``inertia`` (float, summed in double in point order) belongs to
    ``labels`` and the centres they were assigned against; ``n_iter`` assignment rounds were run."""
    labels: torch.Tensor
    centers: torch.Tensor
    inertia: float
    n_iter: int


# ---- checks (all before anything is launched) -----------------------------------------------------------------------------------------
def _check_matrix(name: str, x) -> None:
    if not torch.is_tensor(x):
        raise TypeError(f"{name}: expected a torch tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {x.dtype} is not torch.float32")
    if x.dim() != 2 or x.shape[1] != D:
        raise ValueError(f"{name}: the feature dimension must be {D}, got shape {tuple(x.shape)}")
    if x.shape[0] < 1:
        raise ValueError(f"{name}: no rows")
    if x.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{name}: {x.shape[0]} rows exceed 2^31 - 1")


def _check_device(name: str, x: torch.Tensor) -> None:
    if not x.is_cuda:
        raise ValueError(f"{name}: a tensor on {x.device}; there is no CPU path (the product runs in loco_op_topk on the device)")


def _check_k(name: str, k) -> int:
    if int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"{name} = {k!r} is outside 1 .. {MAX_K}")
    return int(k)


def _check_metric(metric: str) -> int:
    if metric not in METRICS:
        raise ValueError(f"metric = {metric!r} is not one of {sorted(METRICS)}")
    return METRICS[metric]


def _rows(x: torch.Tensor) -> torch.Tensor:
    """x as the kernels take it: unit stride along the features, a row stride that is a multiple of 4, a 16-byte aligned base.  A view
    that already has the form is used where it lies; anything else is copied once."""
    if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.stride(0) >= D and x.stride(0) < 2 ** 23 and x.data_ptr() % 16 == 0:
        return x
    return torch.empty(x.shape, dtype=x.dtype, device=x.device).copy_(x)  # .contiguous() would hand a misaligned dense tensor back


def _exclude_tensor(exclude, M: int, device) -> Optional[torch.Tensor]:
    if exclude is None:
        return None
    t = exclude if torch.is_tensor(exclude) else torch.from_numpy(np.asarray(exclude))
    if t.dim() != 1 or t.shape[0] != M:
        raise ValueError(f"exclude: expected one key index per query ({M}), got shape {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"exclude: dtype {t.dtype} is not an integer type")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


# ---- the launches ---------------------------------------------------------------------------------------------------------------------
def row_norm2(x: torch.Tensor) -> torch.Tensor:
    """f32 [rows]: the squared norm of every row, summed in double in one written order and rounded once (``loco_op_row_norm2``)."""
    _check_matrix("x", x)
    _check_device("x", x)
    x = _rows(x)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().loco_op_row_norm2(x.data_ptr(), x.stride(0), x.shape[0], D, out.data_ptr(), _stream(x.device)), "loco_op_row_norm2")
    return out


def slab_rows(M: int, N: int, k: int, scratch_cap: int) -> int:
    """Queries per launch such that the (query, chunk) records stay under ``scratch_cap`` bytes: a multiple of 128 where that many fit."""
    per_row = -(-N // _CHUNK) * k * 8
    rows = max(1, int(scratch_cap) // per_row)
    rows = min(rows, (2 ** 31 - 1) // -(-N // _CHUNK) * 128)  # workgroups of one launch
    if rows >= 128:
        rows -= rows % 128
    return min(rows, M)


def _topk(Q, K, k, metric_id, exclude, qn2, kn2, scratch_cap) -> TopK:
    lib = _lib.load()
    M, N = Q.shape[0], K.shape[0]
    dev = Q.device
    values = torch.empty((M, k), dtype=torch.float32, device=dev)
    indices = torch.empty((M, k), dtype=torch.int32, device=dev)
    step = slab_rows(M, N, k, scratch_cap)
    need = int(lib.loco_topk_scratch_bytes(step, N, k))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = _stream(dev)
        for a in range(0, M, step):
            b = min(M, a + step)
            _lib.check(lib.loco_op_topk(Q[a:b].data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0),
                                        qn2[a:b].data_ptr() if qn2 is not None else None, kn2.data_ptr() if kn2 is not None else None,
                                        exclude[a:b].data_ptr() if exclude is not None else None, b - a, N, D, k, metric_id,
                                        values[a:b].data_ptr(), indices[a:b].data_ptr(), scratch.data_ptr(), need, stream), "loco_op_topk")
    return TopK(values, indices)


def topk(queries: torch.Tensor, keys: torch.Tensor, k: int = 10, metric: str = "cosine", exclude=None,
         scratch_cap: Optional[int] = None) -> TopK:
    """The ``k`` best keys of every query under ``metric``, best first, ties towards the lower key index.  ``exclude`` (one key index
    per query, -1 for none) names a key that is not a candidate: the query itself for self-similarity, the held-out item for
    leave-one-out.  No M x N buffer is allocated: the launch keeps ``8 M ceil(N / 1024) k`` bytes of records, and queries are split
    into slabs so that this stays under ``scratch_cap`` (default ``SCRATCH_CAP`` = 1 GiB); the split changes no result."""
    _check_matrix("queries", queries)
    _check_matrix("keys", keys)
    k = _check_k("k", k)
    metric_id = _check_metric(metric)
    if exclude is not None and not torch.is_tensor(exclude):
        exclude = np.asarray(exclude)
    if exclude is not None and (exclude.ndim != 1 or exclude.shape[0] != queries.shape[0]):
        raise ValueError(f"exclude: expected one key index per query ({queries.shape[0]}), got shape {tuple(exclude.shape)}")
    cap = SCRATCH_CAP if scratch_cap is None else int(scratch_cap)
    if cap < 1:
        raise ValueError(f"scratch_cap = {scratch_cap!r} must be positive")
    _check_device("queries", queries)
    _check_device("keys", keys)
    if keys.device != queries.device:
        raise ValueError(f"keys: on {keys.device}, queries on {queries.device}")
    if int(_lib.load().loco_topk_max_k()) != MAX_K:
        raise ImportError("neighbors.MAX_K differs from the library's loco_topk_max_k(); rebuild the library")
    Q, K = _rows(queries), _rows(keys)
    ex = _exclude_tensor(exclude, Q.shape[0], Q.device)
    qn2 = kn2 = None
    if metric_id != METRICS["dot"]:
        kn2 = row_norm2(K)
        qn2 = kn2 if Q is K else row_norm2(Q)
    return _topk(Q, K, k, metric_id, ex, qn2, kn2, cap)


def group_mean(rows: torch.Tensor, offsets: torch.Tensor, index: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """(out f32 [G, 768], count i32 [G]): ``out[g]`` = the mean of ``rows[index[j]]`` (``index`` None: ``rows[j]``) over
    ``j in [offsets[g], offsets[g + 1])``, sums in double in an order that depends on the group's size alone, rounded to fp32 once
    (``loco_op_group_mean``).  ``offsets`` int64 [G + 1] on the device.  An empty group leaves its row of ``out`` as it was (zeros when
    ``out`` is not given) and has count 0."""
    _check_matrix("rows", rows)
    if offsets.dim() != 1 or offsets.shape[0] < 2 or offsets.dtype != torch.int64:
        raise ValueError(f"offsets: expected int64 [G + 1] with G >= 1, got {offsets.dtype} {tuple(offsets.shape)}")
    G = offsets.shape[0] - 1
    if index is not None and (index.dim() != 1 or index.dtype != torch.int32):
        raise ValueError(f"index: expected int32 [n], got {index.dtype} {tuple(index.shape)}")
    if out is not None:
        _check_matrix("out", out)
        if out.shape[0] != G or not out.is_contiguous():
            raise ValueError(f"out: expected a contiguous [{G}, {D}] tensor, got {tuple(out.shape)}")
    _check_device("rows", rows)
    dev = rows.device
    rows = _rows(rows)
    offsets = offsets.to(dev).contiguous()
    index = index.to(dev).contiguous() if index is not None else None
    if index is not None:  # the kernel checks what index holds, not how long it is
        lo, hi = (int(v) for v in torch.stack([offsets[0], offsets[-1]]).cpu().tolist())
        if lo < 0 or hi > index.shape[0]:
            raise ValueError(f"offsets: [{lo}, {hi}) leaves index's {index.shape[0]} entries")
    if out is None:
        out = torch.zeros((G, D), dtype=torch.float32, device=dev)
    count = torch.empty(G, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().loco_op_group_mean(rows.data_ptr(), rows.stride(0), rows.shape[0], index.data_ptr() if index is not None else None,
                                                  offsets.data_ptr(), G, D, out.data_ptr(), out.stride(0), count.data_ptr(), _stream(dev)),
                   "loco_op_group_mean")
    return out, count


# ---- what stands on topk --------------------------------------------------------------------------------------------------------------
def hits_at(indices: torch.Tensor, partner: torch.Tensor, ks: Sequence[int]) -> dict:
    """{k: share of rows whose partner is among the row's first k indices} (a pure function of ``topk``'s indices)."""
    hit = indices.to(torch.int64) == partner.to(torch.int64).reshape(-1, 1)
    shares = torch.stack([hit[:, :k].any(dim=1).to(torch.float64).mean() for k in ks]).cpu().tolist()
    return {int(k): float(s) for k, s in zip(ks, shares)}


def recall_at_k(queries: torch.Tensor, keys: torch.Tensor, ks: Sequence[int] = (1, 5, 10), partner=None, metric: str = "cosine") -> dict:
    """{k: share of queries whose partner key (default: the key of the query's own index) is among its k best}."""
    ks = [_check_k("ks entry", k) for k in ks]
    if not ks:
        raise ValueError("ks: empty")
    M = queries.shape[0] if torch.is_tensor(queries) and queries.dim() == 2 else 0
    if partner is not None:
        partner = partner if torch.is_tensor(partner) else torch.from_numpy(np.asarray(partner))
        if partner.dim() != 1 or partner.shape[0] != M:
            raise ValueError(f"partner: expected one key index per query ({M}), got shape {tuple(partner.shape)}")
    top = topk(queries, keys, max(ks), metric)
    if partner is None:
        partner = torch.arange(M, device=queries.device)
    return hits_at(top.indices, partner.to(queries.device), ks)


def vote(neighbour_labels: torch.Tensor, n_classes: int) -> torch.Tensor:
    """int64 [M]: the most frequent class among each row's neighbour labels ([M, k], -1 = no neighbour), ties to the LOWEST class id
    (class 0 where a row has no neighbour at all).  A pure function; works where the tensor lives."""
    lab = neighbour_labels.to(torch.int64)
    M = lab.shape[0]
    valid = lab >= 0
    votes = torch.zeros((M, n_classes), dtype=torch.int64, device=lab.device)
    votes.scatter_add_(1, lab.clamp(min=0), valid.to(torch.int64))
    # one key per (votes, class): more votes first, then the lower class id -- no two entries of a row compare equal
    key = votes * n_classes + (n_classes - 1 - torch.arange(n_classes, device=lab.device))
    return key.argmax(dim=1)


def knn_classify(train: torch.Tensor, labels, queries: torch.Tensor, k: int = 10, n_classes: int = 101, exclude=None,
                 metric: str = "cosine") -> torch.Tensor:
    """int64 [M] on the device: the majority class among each query's ``k`` nearest rows of ``train``, ties to the lowest class id.
    ``labels``: one class id in [0, n_classes) per row of ``train``.  ``exclude`` as in ``topk`` (leave-one-out: ``arange(N)``)."""
    labels = labels if torch.is_tensor(labels) else torch.from_numpy(np.asarray(labels))
    if torch.is_tensor(train) and train.dim() == 2 and (labels.dim() != 1 or labels.shape[0] != train.shape[0]):
        raise ValueError(f"labels: expected one class per row of train ({train.shape[0]}), got shape {tuple(labels.shape)}")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"labels: dtype {labels.dtype} is not an integer type")
    if n_classes < 1:
        raise ValueError(f"n_classes = {n_classes} must be >= 1")
    if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= n_classes):
        raise ValueError(f"labels: values outside 0 .. n_classes - 1 = {n_classes - 1}")
    top = topk(queries, train, k, metric, exclude)
    lab = labels.to(device=top.indices.device, dtype=torch.int64)
    idx = top.indices.to(torch.int64)
    neigh = torch.where(idx >= 0, lab[idx.clamp(min=0)], torch.full_like(idx, -1))
    return vote(neigh, int(n_classes))


def pairs_from_topk(values: torch.Tensor, indices: torch.Tensor, top_k: int):
    """(pairs int64 [T, 2] with i < j, scores f32 [T]), T <= top_k: the rows' (row, neighbour) entries as unordered pairs, each pair
    once -- with the score of the row of its LOWER index where both rows list it -- by (score desc, i asc, j asc).  A pure function of
    ``topk``'s output."""
    M, k = indices.shape
    dev = indices.device
    rows = torch.arange(M, device=dev, dtype=torch.int64).reshape(-1, 1).expand(M, k).reshape(-1)
    cols = indices.to(torch.int64).reshape(-1)
    vals = values.reshape(-1)
    keep = (cols >= 0) & (cols != rows)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    i, j = torch.minimum(rows, cols), torch.maximum(rows, cols)
    span = int(max(M, int(indices.max()) + 1 if indices.numel() else 1))
    order = torch.argsort((i * span + j) * 2 + (rows != i).to(torch.int64))
    i, j, vals = i[order], j[order], vals[order]
    key = i * span + j
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    i, j, vals = i[first], j[first], vals[first]  # ascending (i, j)
    best = torch.sort(vals, descending=True, stable=True).indices[:top_k]
    return torch.stack([i[best], j[best]], dim=1), vals[best]


def mine_pairs(vecs: torch.Tensor, top_k: int = 10, metric: str = "cosine"):
    """Notebook 3's pair loop without the N x N matrix: the ``top_k`` best-scoring pairs of distinct rows, (pairs int64 [T, 2] with
    i < j, scores f32 [T]) on the device, best first.  Every row's ``top_k`` best other rows are found with ``topk`` (a pair among the
    ``top_k`` best of all pairs is among the ``top_k`` best of both its rows); a pair's score is the one computed with its lower index as
    the query."""
    top_k = _check_k("top_k", top_k)
    _check_matrix("vecs", vecs)
    _check_metric(metric)
    _check_device("vecs", vecs)
    me = torch.arange(vecs.shape[0], dtype=torch.int32, device=vecs.device)
    top = topk(vecs, vecs, top_k, metric, exclude=me)
    return pairs_from_topk(top.values, top.indices, top_k)


def cluster_purity(labels, classes) -> float:
    """The share of points that carry their cluster's most common class.  A pure function; works where the tensors live."""
    labels = labels if torch.is_tensor(labels) else torch.from_numpy(np.asarray(labels))
    classes = classes if torch.is_tensor(classes) else torch.from_numpy(np.asarray(classes))
    if labels.dim() != 1 or classes.dim() != 1 or labels.shape[0] != classes.shape[0] or labels.shape[0] == 0:
        raise ValueError(f"cluster_purity: labels {tuple(labels.shape)} and classes {tuple(classes.shape)} must be one non-empty length")
    lab = labels.to(torch.int64)
    cls = classes.to(device=lab.device, dtype=torch.int64)
    if int(lab.min()) < 0 or int(cls.min()) < 0:
        raise ValueError("cluster_purity: negative label or class")
    n_cls = int(cls.max()) + 1
    table = torch.bincount(lab * n_cls + cls, minlength=(int(lab.max()) + 1) * n_cls).reshape(-1, n_cls)
    return float(table.max(dim=1).values.sum().item()) / float(lab.shape[0])


def draw_init(N: int, n_clusters: int, seed: int) -> np.ndarray:
    """``n_clusters`` distinct rows of N drawn with ``numpy.random.Generator(Philox(seed))``."""
    return np.random.Generator(np.random.Philox(int(seed))).choice(N, size=n_clusters, replace=False).astype(np.int64)


def kmeans(X: torch.Tensor, n_clusters: int = 18, iters: int = 50, init=None, seed: int = 0, tol: float = 0.0,
           on_round: Optional[Callable] = None) -> KMeansResult:
    """Lloyd's algorithm on the device.  ``init``: ``n_clusters`` row indices of X (they may repeat), or None for ``draw_init``.
    A round assigns every point with ``topk(X, centers, 1, "l2")`` -- equal distances go to the lower cluster -- and sums the negated
    top-1 values in double in point order into ``inertia``; if no label changed since the round before, it stops there.  Otherwise the
    centres become the means of their points (``loco_op_group_mean`` over the points stably sorted by label; an empty cluster keeps
    its centre), and it stops after ``iters`` rounds, or when ``tol > 0`` and the summed squared centre shift is at most ``tol``.
    ``on_round(round, labels, centers, inertia)`` sees every round's assignment and the centres it was made against.  For one ``init``
    the result is bit-reproducible."""
    _check_matrix("X", X)
    N = X.shape[0]
    if int(n_clusters) != n_clusters or n_clusters < 1:
        raise ValueError(f"n_clusters = {n_clusters!r} must be a positive integer")
    if n_clusters > N:
        raise ValueError(f"n_clusters = {n_clusters} exceeds the {N} points of X")
    if iters < 1:
        raise ValueError(f"iters = {iters} must be >= 1")
    if init is not None:
        init = np.asarray(init.cpu() if torch.is_tensor(init) else init)
        if init.ndim != 1 or init.shape[0] != n_clusters or init.dtype.kind not in "iu":
            raise ValueError(f"init: expected {n_clusters} integer row indices, got shape {init.shape} of {init.dtype}")
        if init.min() < 0 or init.max() >= N:
            raise ValueError(f"init: a row index outside 0 .. {N - 1}")
    _check_device("X", X)
    if init is None:
        init = draw_init(N, int(n_clusters), seed)
    dev = X.device
    X = _rows(X)
    C = int(n_clusters)
    centers = X[torch.from_numpy(init.astype(np.int64)).to(dev)].contiguous()
    xn2 = row_norm2(X)
    prev = None
    labels, inertia, n_iter = None, float("nan"), 0
    for rnd in range(int(iters)):
        top = _topk(X, centers, 1, METRICS["l2"], None, xn2, row_norm2(centers), SCRATCH_CAP)
        labels = top.indices[:, 0].contiguous()
        inertia = float(np.cumsum(-top.values[:, 0].cpu().numpy().astype(np.float64))[-1])  # sequential: point order
        n_iter = rnd + 1
        if on_round is not None:
            on_round(n_iter, labels, centers.clone(), inertia)
        if prev is not None and torch.equal(labels, prev):
            break
        if rnd + 1 == int(iters):
            break
        order = torch.sort(labels.to(torch.int64), stable=True).indices.to(torch.int32)
        offsets = torch.zeros(C + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(torch.bincount(labels.to(torch.int64), minlength=C), dim=0)
        old = centers.clone() if tol > 0 else None
        group_mean(X, offsets, order, out=centers)
        prev = labels
        if old is not None and float(((centers.double() - old.double()) ** 2).sum().item()) <= tol:
            break
    return KMeansResult(labels=labels, centers=centers, inertia=inertia, n_iter=n_iter)
