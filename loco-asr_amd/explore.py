"""Which embeddings are close to which: ``python -m loco-asr_amd.explore --folder extracted/speecht5_base --splits devel --queries audio
--keys text --k 1 5 10 [--knn 10] [--kmeans 18] [--pairs 10] [--metric cosine] --out report.json``.

Reads both modalities of the given splits (the reference's pickle folders, ``extract.py``'s output) into device-resident stores,
matches the items by id -- ids present on one side only are named once on stderr and dropped --, mean-pools every clip
(``EmbeddingStore.pooled``) and writes ONE JSON object:

* ``recall``: per direction (``"audio->text"``, ``"text->audio"``) and per k, the share of items whose own counterpart is among the k
  nearest of the other modality;
* ``knn_accuracy``: per modality, leave-one-out accuracy of the intent labels under a ``--knn`` nearest-neighbour vote (ties to the
  lowest class id; ``--knn 0`` leaves it out);
* with ``--kmeans C``: per modality ``inertia``, ``n_iter`` and ``purity`` of C clusters against the intent labels;
* with ``--pairs P``: the best P pairs of distinct utterances of the queries' modality as ``[id, id, score]``, best first.

Everything is computed on the device by neighbors.py (csrc/neighbors.hip); no N x N matrix is formed.  The rules -- ties to the lower
index, NaN scores dropped, cosine with normalize's eps -- are this project's own, written down in include/loco_asr.h; nothing here
is validated against sentence-transformers or scikit-learn.  Exit code 1 when no id matched.
"""
from __future__ import annotations

import argparse
import json
import sys


def parser():
    ap = argparse.ArgumentParser(prog="python -m loco-asr_amd.explore", description=__doc__.split("\n\n")[0])
    ap.add_argument("--folder", required=True, help="root of the extracted embeddings: {folder}/{split}/{modality}/*.pickle")
    ap.add_argument("--splits", nargs="+", default=["devel"], help="splits to read (default: devel)")
    ap.add_argument("--queries", default="audio", help="modality of the queries (default: audio)")
    ap.add_argument("--keys", default="text", help="modality of the keys (default: text)")
    ap.add_argument("--k", nargs="+", type=int, default=[1, 5, 10], help="recall at these k, each 1 .. 16 (default: 1 5 10)")
    ap.add_argument("--knn", type=int, default=10, help="neighbours of the leave-one-out intent vote, 1 .. 16; 0 leaves it out (default: 10)")
    ap.add_argument("--kmeans", type=int, default=0, metavar="C", help="also cluster each modality into C clusters (Lloyd's algorithm)")
    ap.add_argument("--kmeans-iters", type=int, default=50, help="rounds of k-means at the most (default: 50)")
    ap.add_argument("--pairs", type=int, default=0, metavar="P", help="also list the P best pairs of distinct utterances, 1 .. 16")
    ap.add_argument("--metric", choices=["cosine", "dot", "l2"], default="cosine", help="score of recall, kNN and pairs (default: cosine)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the k-means initial centres (default: 0)")
    ap.add_argument("--device", default="cuda", help="torch device (default: cuda)")
    ap.add_argument("--workers", type=int, default=8, help="threads that read the pickles (default: 8)")
    ap.add_argument("--out", required=True, metavar="FILE", help="the JSON report ('-' for stdout)")
    return ap


def check_args(args, ap):
    from .neighbors import MAX_K
    for k in args.k:
        if not 1 <= k <= MAX_K:
            ap.error(f"--k {k} is outside 1 .. {MAX_K}")
    if args.knn and not 1 <= args.knn <= MAX_K:
        ap.error(f"--knn {args.knn} is outside 1 .. {MAX_K} (0 leaves it out)")
    if args.pairs and not 1 <= args.pairs <= MAX_K:
        ap.error(f"--pairs {args.pairs} is outside 1 .. {MAX_K}")
    if args.kmeans < 0 or args.kmeans_iters < 1:
        ap.error("--kmeans must be >= 0 and --kmeans-iters >= 1")
    if args.queries == args.keys:
        ap.error(f"--queries and --keys are both {args.queries!r}")


def match_ids(ids_a, ids_b, name_a, name_b, err=sys.stderr):
    """(rows of a, rows of b) of the ids both sides hold, in a's order; the ids of one side only are named once on ``err``."""
    where_b = {}
    for n, u in enumerate(ids_b):
        where_b.setdefault(u, n)
    seen, rows_a, rows_b, only_a = set(), [], [], []
    for n, u in enumerate(ids_a):
        if u in seen:
            continue
        seen.add(u)
        if u in where_b:
            rows_a.append(n)
            rows_b.append(where_b[u])
        else:
            only_a.append(u)
    only_b = [u for u in where_b if u not in seen]
    for name, only in ((name_a, only_a), (name_b, only_b)):
        if only:
            print(f"dropped {len(only)} ids present in {name} only: {' '.join(str(u) for u in only)}", file=err)
    return rows_a, rows_b


def load_pooled(args):
    """{modality: (ids, vecs f32 [n, 768], classes int64 [n])} of the matched items, both in the queries' order."""
    import torch
    from .embedding_store import EmbeddingStore
    stores = {m: EmbeddingStore.from_folders(args.folder, m, args.splits, args.device, workers=args.workers) for m in (args.queries, args.keys)}
    rows_q, rows_k = match_ids(stores[args.queries].ids, stores[args.keys].ids, args.queries, args.keys)
    out = {}
    for m, rows in ((args.queries, rows_q), (args.keys, rows_k)):
        st = stores[m]
        sel = torch.tensor(rows, dtype=torch.int64, device=st.device)
        if not rows:
            out[m] = ([], None, None)
            continue
        out[m] = ([st.ids[r] for r in rows], st.pooled("average")[sel].contiguous(), st.targets[sel].argmax(dim=1))
    return out


def recall_report(args, data):
    from . import neighbors as nb
    (_, q, _), (_, k, _) = data[args.queries], data[args.keys]
    fmt = lambda r: {str(kk): v for kk, v in r.items()}  # noqa: E731
    return {f"{args.queries}->{args.keys}": fmt(nb.recall_at_k(q, k, args.k, metric=args.metric)),
            f"{args.keys}->{args.queries}": fmt(nb.recall_at_k(k, q, args.k, metric=args.metric))}


def knn_report(args, data):
    import torch
    from . import neighbors as nb
    out = {}
    for m, (_, vecs, classes) in data.items():
        me = torch.arange(vecs.shape[0], dtype=torch.int32, device=vecs.device)
        pred = nb.knn_classify(vecs, classes, vecs, k=args.knn, n_classes=int(classes.max()) + 1, exclude=me, metric=args.metric)
        out[m] = float((pred == classes).to(torch.float64).mean().item())
    return out


def kmeans_report(args, data):
    from . import neighbors as nb
    out = {}
    for m, (_, vecs, classes) in data.items():
        km = nb.kmeans(vecs, n_clusters=args.kmeans, iters=args.kmeans_iters, seed=args.seed)
        out[m] = {"inertia": km.inertia, "n_iter": km.n_iter, "purity": nb.cluster_purity(km.labels, classes)}
    return out


def pairs_report(args, data):
    from . import neighbors as nb
    ids, vecs, _ = data[args.queries]
    pairs, scores = nb.mine_pairs(vecs, top_k=args.pairs, metric=args.metric)
    return [[ids[i], ids[j], float(s)] for (i, j), s in zip(pairs.cpu().tolist(), scores.cpu().tolist())]


def write_report(args, report):
    text = json.dumps(report, indent=1)
    if args.out == "-":
        print(text)
    else:
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    check_args(args, ap)
    data = load_pooled(args)
    n = len(data[args.queries][0])
    if n == 0:
        print(f"no id is present in both {args.queries} and {args.keys}", file=sys.stderr)
        return 1
    report = {"folder": args.folder, "splits": args.splits, "queries": args.queries, "keys": args.keys, "items": n, "metric": args.metric,
              "recall": recall_report(args, data)}
    if args.knn:
        report["knn_k"] = args.knn
        report["knn_accuracy"] = knn_report(args, data)
    if args.kmeans:
        if args.kmeans > n:
            ap.error(f"--kmeans {args.kmeans} exceeds the {n} matched items")
        report["kmeans"] = kmeans_report(args, data)
    if args.pairs:
        report["pairs"] = pairs_report(args, data)
    write_report(args, report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
