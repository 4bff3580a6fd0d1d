"""Embedding neighbours on the MI355X (csrc/neighbors.hip) against the numpy restatement of the rules (tests/neighbors_ref.py).

Exact tier: entries from {-2 .. 2}, so every dot product and squared norm is an integer below 2^24 and exact in fp32 in any order;
`dot` and `l2` results equal the restatement bit for bit, ties (they are everywhere with this alphabet) included.
Cosine tier: |values - restatement| <= 1e-4, derived and not measured: 768 * 2^-24 = 4.6e-5 bounds the fp32 dot-product error of unit
vectors in any order, plus the handful of scaling roundings.  Measured on the MI355X (profiles/neighbors_parity.jsonl): max
|values - restatement| = 3.0e-7 at k = 5 and 16, 2.7e-7 at k = 1; the k-means inertia is within 1.1e-7 relative of the float64 scores'
and the centres equal the restatement's.  The figures are recorded by the tests before they assert."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import neighbors_ref as ref
from conftest import ROOT, record_figure

pytestmark = pytest.mark.gpu

nb = importlib.import_module("loco-asr_amd.neighbors")
_lib = importlib.import_module("loco-asr_amd._lib")
store_mod = importlib.import_module("loco-asr_amd.embedding_store")
sink = importlib.import_module("loco-asr_amd.sink")

DEV = "cuda:0"
D = 768
GUARD = 64
PAT_F, PAT_I = -12345.5, -77777
MS = (1, 127, 128, 129, 300)
NS = (1, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 2049)
KS = (1, 5, 16)
METRIC_ID = {"dot": 0, "cosine": 1, "l2": 2}


def strided(x, ld):
    """x [rows, 768] as a view with row stride ld into a buffer whose other columns hold NaN: reading past column 767 shows."""
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :D] = torch.from_numpy(x).to(DEV)
    return buf[:, :D]


@pytest.fixture(scope="module")
def exact():
    """The integer inputs (strided on the device) and the restatement's score matrices, computed once and left unchanged."""
    Q, K = ref.integer_input()
    exclude = np.random.Generator(np.random.Philox(11)).integers(-1, 2049, 300).astype(np.int32)
    exclude[:4] = [0, -1, 1, 0]
    return {"Q": Q, "K": K, "Qd": strided(Q, 772), "Kd": strided(K, 800), "exclude": exclude,
            "S": {m: ref.scores(Q, K, m) for m in ("dot", "l2")}}


@pytest.fixture(scope="module")
def cosine():
    Q, K = ref.cosine_input()
    S = ref.scores(Q, K, "cosine")
    return {"Q": Q, "K": K, "Qd": torch.from_numpy(Q).to(DEV), "Kd": torch.from_numpy(K).to(DEV), "S": S}


def guarded(n, dtype, pattern):
    buf = torch.full((n + 2 * GUARD,), pattern, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n, pattern):
    return bool((buf[:GUARD] == pattern).all()) and bool((buf[GUARD + n:] == pattern).all())


def raw_topk(Q, K, k, metric, exclude=None):
    """loco_op_topk through the C ABI with guard bands on both sides of values, indices and scratch: (values, indices) on the host."""
    lib = _lib.load()
    M, N = Q.shape[0], K.shape[0]
    qn2 = kn2 = None
    if metric != "dot":
        qn2, kn2 = nb.row_norm2(Q), nb.row_norm2(K)
    vbuf, v = guarded(M * k, torch.float32, PAT_F)
    ibuf, i = guarded(M * k, torch.int32, PAT_I)
    need = int(lib.loco_topk_scratch_bytes(M, N, k))
    assert need == 8 * M * ((N + 1023) // 1024) * k and need % 4 == 0
    sbuf, s = guarded(need // 4, torch.int32, PAT_I)
    ex = torch.from_numpy(exclude).to(DEV) if exclude is not None else None
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.loco_op_topk(Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), qn2.data_ptr() if qn2 is not None else None,
                          kn2.data_ptr() if kn2 is not None else None, ex.data_ptr() if ex is not None else None, M, N, D, k, METRIC_ID[metric],
                          v.data_ptr(), i.data_ptr(), s.data_ptr(), need, stream)
    _lib.check(rc, "loco_op_topk")
    torch.cuda.synchronize()
    assert guards_intact(vbuf, M * k, PAT_F) and guards_intact(ibuf, M * k, PAT_I) and guards_intact(sbuf, need // 4, PAT_I)
    return v.reshape(M, k).cpu().numpy(), i.reshape(M, k).cpu().numpy()


def assert_bit_equal(v, i, want_v, want_i, what):
    assert np.array_equal(i, want_i), what
    assert np.array_equal(v.view(np.uint32), want_v.astype(np.float32).view(np.uint32)), what


# ---- exact tier -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_exact_tier_equals_the_restatement_bit_for_bit(exact, N):
    """Every M, k, metric, with and without exclude, at one N: values and indices, ties and the (-inf, -1) tail included."""
    for metric in ("dot", "l2"):
        for with_exclude in (False, True):
            ex_all = exact["exclude"] if with_exclude else None
            want_v, want_i = ref.select(exact["S"][metric][:, :N], 16, ex_all)  # a prefix of it is the answer for a smaller M or k
            for M in MS:
                ex = np.ascontiguousarray(ex_all[:M]) if with_exclude else None
                for k in KS:
                    v, i = raw_topk(exact["Qd"][:M], exact["Kd"][:N], k, metric, ex)
                    assert_bit_equal(v, i, want_v[:M, :k], want_i[:M, :k], (metric, with_exclude, M, N, k))
                    if N < k:
                        assert (i[:, N:] == -1).all() and np.isneginf(v[:, N:]).all()
                    if with_exclude:
                        assert not ((i == ex[:, None]) & (i >= 0)).any()


def test_ties_are_everywhere_in_the_exact_tier(exact):
    """The alphabet does what it is there for: most queries' 16 best dot products at N = 2049 hold equal values."""
    want_v, _ = ref.select(exact["S"]["dot"], 16)
    assert np.mean([len(set(r.tolist())) < 16 for r in want_v]) > 0.9


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_a_nan_key_is_never_returned(exact, metric):
    K = exact["K"][:300].copy()
    K[[0, 17, 128, 299], 5] = np.nan
    Kd = strided(K, 772)
    want_v, want_i = ref.topk(exact["Q"][:129], K, 16, metric)
    v, i = raw_topk(exact["Qd"][:129], Kd, 16, metric)
    assert not np.isin(i, [0, 17, 128, 299]).any() and not np.isnan(v).any()
    assert_bit_equal(v, i, want_v, want_i, metric)
    # nothing but NaN keys: no candidate at all
    v, i = raw_topk(exact["Qd"][:3], Kd[:1], 5, metric)
    assert (i == -1).all() and np.isneginf(v).all()


def test_the_python_entry_is_the_c_entry(exact):
    ex = exact["exclude"]
    top = nb.topk(exact["Qd"], exact["Kd"], k=5, metric="l2", exclude=ex)
    v, i = raw_topk(exact["Qd"], exact["Kd"], 5, "l2", ex)
    assert top.values.shape == (300, 5) and top.indices.dtype == torch.int32 and top.values.is_cuda
    assert_bit_equal(top.values.cpu().numpy(), top.indices.cpu().numpy(), v, i, "python vs C")
    shifted = torch.zeros(299 * D + 1, device=DEV)[1:].view(299, D).copy_(exact["Qd"][1:])  # a base that is not 16-byte aligned: copied once
    assert shifted.data_ptr() % 16 != 0
    top2 = nb.topk(shifted, exact["Kd"], k=5, metric="l2", exclude=ex[1:])
    assert torch.equal(top2.indices, top.indices[1:]) and torch.equal(top2.values, top.values[1:])


# ---- cosine tier ----------------------------------------------------------------------------------------------------------------------
def test_cosine_tier_within_1e_4_of_the_restatement(cosine):
    S = cosine["S"]
    worst = {}
    for k in KS:
        want_v, _ = ref.select(S, k)
        top = nb.topk(cosine["Qd"], cosine["Kd"], k=k, metric="cosine")
        v, i = top.values.cpu().numpy().astype(np.float64), top.indices.cpu().numpy()
        err_sorted = float(np.abs(v - want_v).max())  # order statistics are 1-Lipschitz: no exclusion of near ties is needed
        err_own = float(np.abs(np.take_along_axis(S, i.astype(np.int64), axis=1) - v).max())
        worst[k] = (err_sorted, err_own)
        record_figure("neighbors_cosine_tier", M=300, N=2049, k=k, max_abs_err_vs_sorted=err_sorted, max_abs_err_vs_own_score=err_own, bar=1e-4)
        print(f"cosine tier k={k}: |v - ref_sorted| max {err_sorted:.3e}, |S64[i, idx] - v| max {err_own:.3e}")
        assert (i >= 0).all() and (i < 2049).all()
        assert all(len(set(r.tolist())) == k for r in i)
        assert (np.diff(v, axis=1) <= 0).all()  # best first
    for k, (a, b) in worst.items():
        assert a <= 1e-4 and b <= 1e-4, (k, a, b)


def test_cosine_with_exclude_and_a_zero_vector(cosine):
    Q = cosine["Q"][:130].copy()
    Q[7] = 0.0  # a zero vector scores 0 against everything: its neighbours are keys 0 .. k - 1
    K = cosine["K"][:1025]
    ex = np.arange(130, dtype=np.int32)
    top = nb.topk(torch.from_numpy(Q).to(DEV), torch.from_numpy(K).to(DEV), k=5, metric="cosine", exclude=ex)
    v, i = top.values.cpu().numpy(), top.indices.cpu().numpy()
    assert not (i == ex[:, None]).any()
    assert i[7].tolist() == [0, 1, 2, 3, 4] and (v[7] == 0).all()
    want_v, _ = ref.topk(Q, K, 5, "cosine", ex)
    assert np.abs(v - want_v).max() <= 1e-4


# ---- independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_a_query_does_not_see_its_batch(cosine, metric):
    """Row 137 of the cosine tier alone, as row 0 and as row 299 of the batch, in its own place, and through a cap that forces three
    slabs: the same 2 k words."""
    Qd, Kd, k, row = cosine["Qd"], cosine["Kd"], 16, 137
    ex = torch.full((300,), -1, dtype=torch.int32, device=DEV)
    ex[row] = 3

    def words(top, r):
        return top.values[r].view(torch.int32).tolist() + top.indices[r].tolist()

    base = nb.topk(Qd, Kd, k=k, metric=metric, exclude=ex)
    want = words(base, row)
    alone = nb.topk(Qd[row:row + 1], Kd, k=k, metric=metric, exclude=ex[row:row + 1])
    assert words(alone, 0) == want
    for at in (0, 299):
        Q2, ex2 = Qd.clone(), ex.clone()
        Q2[at], ex2[at] = Qd[row], 3
        Q2[row], ex2[row] = Qd[at], -1
        assert words(nb.topk(Q2, Kd, k=k, metric=metric, exclude=ex2), at) == want
    cap = 100 * 3 * k * 8
    assert nb.slab_rows(300, 2049, k, cap) == 100  # three slabs: row 137 is row 37 of the second
    slabbed = nb.topk(Qd, Kd, k=k, metric=metric, exclude=ex, scratch_cap=cap)
    assert torch.equal(slabbed.indices, base.indices) and torch.equal(slabbed.values.view(torch.int32), base.values.view(torch.int32))
    assert 3 not in base.indices[row].tolist()


# ---- row norms and group mean ---------------------------------------------------------------------------------------------------------
def test_row_norms(exact, cosine):
    got = nb.row_norm2(exact["Kd"]).cpu().numpy()
    assert np.array_equal(got, ref.norm2(exact["K"]).astype(np.float32))  # integers: exact
    got = nb.row_norm2(cosine["Kd"]).cpu().numpy()
    want = ref.norm2(cosine["K"]).astype(np.float32)  # double sum, one rounding: at most the rounding's own ulp apart
    assert (np.abs(got - want) <= np.spacing(want)).all()


GROUP_SIZES = (0, 1, 2, 63, 64, 65, 1000, 0)


@pytest.fixture(scope="module")
def groups():
    g = np.random.Generator(np.random.Philox(20250104))
    n = sum(GROUP_SIZES)
    rows = (g.standard_normal((n + 40, D)) * 3.0 + 1.0).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.int64)
    index = g.integers(0, n + 40, n).astype(np.int32)  # any rows, repeats included
    return rows, offsets, index


@pytest.mark.parametrize("with_index", [False, True])
def test_group_mean_within_one_ulp_and_leaves_empty_groups_alone(groups, with_index):
    rows, offsets, index = groups
    G = len(GROUP_SIZES)
    lib = _lib.load()
    rows_d = strided(rows, 776)
    obuf, out = guarded(G * D, torch.float32, PAT_F)
    cbuf, count = guarded(G, torch.int32, PAT_I)
    off_d = torch.from_numpy(offsets).to(DEV)
    idx_d = torch.from_numpy(index).to(DEV) if with_index else None
    rc = lib.loco_op_group_mean(rows_d.data_ptr(), rows_d.stride(0), rows.shape[0], idx_d.data_ptr() if with_index else None, off_d.data_ptr(), G, D,
                                out.data_ptr(), D, count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "loco_op_group_mean")
    torch.cuda.synchronize()
    assert guards_intact(obuf, G * D, PAT_F) and guards_intact(cbuf, G, PAT_I)
    got = out.reshape(G, D).cpu().numpy()
    want, want_count = ref.group_mean(rows, offsets, index if with_index else None, out=np.full((G, D), PAT_F, np.float32))
    assert count.cpu().tolist() == want_count.tolist() == list(GROUP_SIZES)
    for g, size in enumerate(GROUP_SIZES):
        if size == 0:
            assert (got[g] == PAT_F).all()  # untouched
        else:
            assert (np.abs(got[g] - want[g]) <= np.spacing(np.abs(want[g]))).all(), g
    # the Python entry: the same bits; an empty group's row is zero when no `out` is given
    out2, count2 = nb.group_mean(rows_d, off_d, idx_d)
    assert torch.equal(count2, count)
    nonempty = torch.tensor([s > 0 for s in GROUP_SIZES], device=DEV)
    assert torch.equal(out2[nonempty], out.reshape(G, D)[nonempty]) and bool((out2[~nonempty] == 0).all())


def test_store_pooled_is_the_group_mean(groups):
    rows, _, _ = groups
    lengths = [1, 7, 64, 130, 3]
    embs, at = [], 0
    for n in lengths:
        embs.append(rows[at:at + n])
        at += n
    store = store_mod.EmbeddingStore.from_arrays([f"u{i}" for i in range(5)], embs, [np.eye(101)[i] for i in range(5)], device=DEV)
    vecs = store.pooled("average")
    assert vecs.shape == (5, D) and vecs.dtype == torch.float32 and vecs.is_cuda
    want = np.stack([e.astype(np.float64).mean(axis=0).astype(np.float32) for e in embs])
    assert (np.abs(vecs.cpu().numpy() - want) <= np.spacing(np.abs(want))).all()
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=DEV)
    assert torch.equal(vecs, nb.group_mean(store.rows, offsets)[0])


# ---- k-means --------------------------------------------------------------------------------------------------------------------------
def test_kmeans_follows_the_restatement_round_by_round():
    X, init, planted = ref.kmeans_input()
    rounds, final = ref.kmeans(X, init, 50)
    for r in rounds:  # the precondition (tests/test_neighbors_ref.py asserts it on the CPU as well)
        assert r["margin"] > ref.kmeans_margin_bound(X, r["centers"])
    Xd = torch.from_numpy(X).to(DEV)
    seen = []
    km = nb.kmeans(Xd, n_clusters=8, iters=50, init=init, on_round=lambda n, lab, cen, inertia: seen.append((n, lab.cpu().numpy(), cen, inertia)))
    assert km.n_iter == len(rounds) == len(seen) == 2
    for (n, lab, cen, inertia), r in zip(seen, rounds):
        assert np.array_equal(lab, r["labels"]), n
        c = cen.cpu().numpy()
        assert (np.abs(c - r["centers"]) <= np.spacing(np.abs(r["centers"]))).all(), n
        # the rule: the negated top-1 values, summed in double in point order
        top1 = nb.topk(Xd, cen, k=1, metric="l2").values[:, 0].cpu().numpy()
        assert abs(inertia - ref.inertia_of(top1)) <= 1e-12 * abs(inertia), n
        # and against the float64 scores: every fp32 score is within the margin bound of its float64 value
        assert abs(inertia - r["inertia"]) <= X.shape[0] * ref.kmeans_margin_bound(X, r["centers"]), n
        record_figure("neighbors_kmeans_round", round=n, inertia=inertia, inertia_f64_scores=r["inertia"],
                      rel_gap=abs(inertia - r["inertia"]) / r["inertia"], max_center_err_ulp=float((np.abs(c - r["centers"]) / np.spacing(np.abs(r["centers"]))).max()))
    assert np.array_equal(km.labels.cpu().numpy(), planted) and km.labels.dtype == torch.int32
    assert (np.abs(km.centers.cpu().numpy() - final) <= np.spacing(np.abs(final))).all()
    assert km.inertia == seen[-1][3]
    again = nb.kmeans(Xd, n_clusters=8, iters=50, init=init)
    assert torch.equal(again.labels, km.labels) and torch.equal(again.centers.view(torch.int32), km.centers.view(torch.int32))
    assert again.inertia == km.inertia and again.n_iter == km.n_iter
    assert nb.cluster_purity(km.labels, torch.from_numpy(planted).to(DEV)) == 1.0


def test_kmeans_a_repeated_initial_row_leaves_its_second_cluster_empty():
    """Integer-valued points: cluster A is 50 copies of one row, B and C are two rows plus noise from {-1, 0, 1}.  `init` names A's row
    twice.  Both copies tie on every point of A, exactly, in every round -- A's mean is A's row -- and the tie goes to the lower cluster:
    the second copy's cluster stays empty and keeps its centre."""
    g = np.random.Generator(np.random.Philox(20250106))
    a, b, c = (4.0 * g.integers(-2, 3, (3, D))).astype(np.float32)
    X = np.concatenate([np.repeat(a[None], 50, axis=0), b + g.integers(-1, 2, (50, D)), c + g.integers(-1, 2, (50, D))]).astype(np.float32)
    perm = g.permutation(150)
    X, planted = X[perm], (np.arange(150) // 50)[perm]
    first = [int(np.flatnonzero(planted == p)[0]) for p in range(3)]
    init = [first[0], first[1], first[0], first[2]]
    Xd = torch.from_numpy(X).to(DEV)
    km = nb.kmeans(Xd, n_clusters=4, iters=10, init=init)
    labels = km.labels.cpu().numpy()
    assert not (labels == 2).any()
    assert np.array_equal(labels, np.asarray([0, 1, 3])[planted])
    assert torch.equal(km.centers[2], Xd[first[0]]) and torch.equal(km.centers[0], Xd[first[0]])  # kept; and A's mean is A's row
    rounds, final = ref.kmeans(X, init, 10)
    assert km.n_iter == len(rounds) == 2 and np.array_equal(labels, rounds[-1]["labels"])
    assert (np.abs(km.centers.cpu().numpy() - final) <= np.spacing(np.abs(final))).all()
    seeded = nb.kmeans(Xd, n_clusters=4, iters=2, seed=3)
    assert torch.equal(seeded.labels, nb.kmeans(Xd, n_clusters=4, iters=2, init=nb.draw_init(150, 4, 3)).labels)


# ---- what stands on topk --------------------------------------------------------------------------------------------------------------
def test_recall_knn_and_pairs_against_the_restatement(cosine):
    Q, K = cosine["Q"][:129], cosine["K"][:129]
    Qd, Kd = cosine["Qd"][:129], cosine["Kd"][:129]
    Kn = (0.8 * Q + 0.2 * K).astype(np.float32)  # keys that resemble their own query
    Knd = torch.from_numpy(Kn).to(DEV)
    _, idx = ref.topk(Q, Kn, 10, "cosine")
    assert nb.recall_at_k(Qd, Knd, ks=(1, 5, 10)) == ref.recall_at_k(idx, np.arange(129), (1, 5, 10))
    partner = (np.arange(129) + 1) % 129
    assert nb.recall_at_k(Qd, Knd, ks=(1, 10), partner=partner) == ref.recall_at_k(idx, partner, (1, 10))
    labels = np.random.Generator(np.random.Philox(3)).integers(0, 7, 129)
    me = np.arange(129, dtype=np.int32)
    got = nb.knn_classify(Kd, labels, Kd, k=10, n_classes=7, exclude=me).cpu().numpy()
    assert np.array_equal(got, ref.knn_classify(K, labels, K, 10, 7, me))
    pairs, scores = nb.mine_pairs(Kd, top_k=10)
    v, i = ref.topk(K, K, 10, "cosine", me)
    want_pairs, want_scores = ref.pairs_from_topk(v, i, 10)
    assert [tuple(p) for p in pairs.cpu().tolist()] == want_pairs
    assert np.abs(scores.cpu().numpy() - np.asarray(want_scores)).max() <= 1e-4
    S = ref.scores(K, K, "cosine")  # the notebook's loop: every pair i < j, sorted
    brute = sorted(((-S[a, b], a, b) for a in range(129) for b in range(a + 1, 129)))[:10]
    assert want_pairs == [(a, b) for _, a, b in brute]


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def test_explore_cli_reports_what_the_restatement_computes(tmp_path):
    g = np.random.Generator(np.random.Philox(20250105))
    n, n_cls = 24, 4
    base = g.standard_normal((n_cls, D)) + 0.0
    ids = [f"utt{i:02d}" for i in range(n)]
    cls = np.arange(n) % n_cls
    embs = {"audio": [], "text": []}
    for m in ("audio", "text"):
        os.makedirs(tmp_path / "devel" / m)
    for i in range(n):
        own = base[cls[i]] + 0.7 * g.standard_normal(D)
        for m, frames, noise in (("audio", 3 + i % 5, 1.0), ("text", 2 + i % 3, 0.6)):
            e = (own[None, :] + noise * g.standard_normal((frames, D))).astype(np.float32)
            embs[m].append(e)
            sink.write_one(str(tmp_path / "devel" / m), ids[i], e, np.eye(101, dtype=np.int64)[cls[i]])
    sink.write_one(str(tmp_path / "devel" / "audio"), "utt99", embs["audio"][0], np.eye(101, dtype=np.int64)[0])  # no transcript: dropped
    out = tmp_path / "report.json"
    cmd = [sys.executable, "-m", "loco-asr_amd.explore", "--folder", str(tmp_path), "--splits", "devel", "--queries", "audio", "--keys", "text",
           "--k", "1", "5", "10", "--knn", "5", "--kmeans", "4", "--pairs", "3", "--out", str(out)]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "dropped 1 ids present in audio only: utt99" in run.stderr
    rep = json.loads(out.read_text())
    assert rep["items"] == n and rep["queries"] == "audio" and rep["keys"] == "text"
    # the same pooled vectors: the store's, read back
    pooled = {}
    for m in ("audio", "text"):
        store = store_mod.EmbeddingStore.from_arrays(ids, embs[m], [np.eye(101)[c] for c in cls], device=DEV)
        pooled[m] = store.pooled("average").cpu().numpy()
    me = np.arange(n, dtype=np.int32)
    for a, b in (("audio", "text"), ("text", "audio")):
        _, idx = ref.topk(pooled[a], pooled[b], 10, "cosine")
        want = ref.recall_at_k(idx, np.arange(n), (1, 5, 10))
        assert rep["recall"][f"{a}->{b}"] == {str(k): v for k, v in want.items()}
    for m in ("audio", "text"):
        pred = ref.knn_classify(pooled[m], cls, pooled[m], 5, n_cls, me)
        assert rep["knn_accuracy"][m] == float(np.mean(pred == cls))
        assert 0.0 < rep["kmeans"][m]["purity"] <= 1.0 and rep["kmeans"][m]["n_iter"] >= 1 and rep["kmeans"][m]["inertia"] > 0
    v, i = ref.topk(pooled["audio"], pooled["audio"], 3, "cosine", me)
    want_pairs, want_scores = ref.pairs_from_topk(v, i, 3)
    assert [(p[0], p[1]) for p in rep["pairs"]] == [(ids[a], ids[b]) for a, b in want_pairs]
    assert max(abs(p[2] - s) for p, s in zip(rep["pairs"], want_scores)) <= 1e-4
