"""The numpy restatement of the neighbour rules (tests/neighbors_ref.py) checked on its own, and the package's pure functions --
the kNN vote, the pair dedupe, cluster purity -- against it.  No GPU."""
import importlib

import numpy as np
import pytest
import torch

import neighbors_ref as ref

nb = importlib.import_module("loco-asr_amd.neighbors")


def tied_scores(seed, M=7, N=23):
    g = np.random.Generator(np.random.Philox(seed))
    S = g.integers(-2, 3, (M, N)).astype(np.float64)  # five values over 23 columns: ties in every row
    S[1, 4] = np.nan
    S[2, :] = 1.0
    S[3, 5] = -np.inf
    return S


@pytest.mark.parametrize("k", [1, 5, 16, 30])
@pytest.mark.parametrize("with_exclude", [False, True])
def test_select_is_the_brute_force_sort(k, with_exclude):
    S = tied_scores(1)
    exclude = np.asarray([0, 4, 0, -1, 22, 3, -1]) if with_exclude else None
    v, i = ref.select(S, k, exclude)
    bv, bi = ref.brute_force(S, k, exclude)
    assert np.array_equal(i, bi)
    assert np.array_equal(v, bv)
    if with_exclude:
        for r, e in enumerate(exclude):
            assert e < 0 or e not in i[r]
    assert 4 not in i[1]  # the NaN is never a candidate
    if k == 30:  # 23 columns: the tail is (-inf, -1)
        assert (i[0, 23:] == -1).all() and np.isneginf(v[0, 23:]).all()
        assert (i[2, :23] == np.arange(23)).all() or with_exclude  # equal scores: ascending index
        assert 5 in i[3]  # a score of -inf is a candidate, unlike NaN


def test_the_three_metrics_on_a_case_done_by_hand():
    Q = np.zeros((2, ref.D)); K = np.zeros((3, ref.D))
    Q[0, :2] = [3, 4]            # |q0| = 5; q1 is the zero vector
    K[0, :2] = [3, 4]; K[1, :2] = [-4, 3]; K[2, :2] = [6, 8]
    assert np.array_equal(ref.scores(Q, K, "dot"), [[25, 0, 50], [0, 0, 0]])
    np.testing.assert_allclose(ref.scores(Q, K, "cosine"), [[1, 0, 1], [0, 0, 0]], atol=1e-15)  # a zero vector scores 0
    assert np.array_equal(ref.scores(Q, K, "l2"), [[0, -50, -25], [-25, -25, -100]])
    _, i = ref.topk(Q, K, 3, "l2")
    assert i.tolist() == [[0, 2, 1], [0, 1, 2]]  # the tie of row 1 goes to the lower index


def test_group_mean_keeps_the_row_of_an_empty_group():
    rows = np.arange(5 * ref.D, dtype=np.float32).reshape(5, ref.D)
    out = np.full((3, ref.D), 7.0, np.float32)
    got, count = ref.group_mean(rows, [0, 2, 2, 5], out=out)
    assert count.tolist() == [2, 0, 3]
    assert np.array_equal(got[1], out[1])
    assert np.array_equal(got[0], rows[:2].mean(0)) and np.array_equal(got[2], rows[2:].mean(0))
    got, _ = ref.group_mean(rows, [0, 2, 3], index=[4, 4, 0])
    assert np.array_equal(got[0], rows[4]) and np.array_equal(got[1], rows[0])


def test_vote_ties_go_to_the_lowest_class():
    neigh = np.asarray([[3, 1, 3, 1, 2],      # 1 and 3 tie at two votes: 1
                        [4, 4, 0, -1, -1],    # missing neighbours do not vote
                        [2, 1, 0, 5, 6],      # all tie: 0
                        [-1, -1, -1, -1, -1]])
    want = ref.vote(neigh, 7)
    assert want.tolist() == [1, 4, 0, 0]
    assert nb.vote(torch.from_numpy(neigh), 7).tolist() == want.tolist()
    g = np.random.Generator(np.random.Philox(5))
    big = g.integers(-1, 9, (200, 10))
    assert nb.vote(torch.from_numpy(big), 9).tolist() == ref.vote(big, 9).tolist()


def test_pairs_are_unique_ordered_and_scored_from_the_lower_row():
    # four rows, k = 3; row 0 and row 2 list each other with different last bits; (1, 3) is listed by row 3 only
    values = np.asarray([[0.9, 0.5, 0.1], [0.5, 0.4, -np.inf], [0.9000001, 0.4, 0.2], [0.95, 0.2, 0.1]], np.float32)
    indices = np.asarray([[2, 1, 3], [0, 2, -1], [0, 1, 3], [1, 2, 0]], np.int32)
    pairs, sc = ref.pairs_from_topk(values, indices, 10)
    assert pairs == [(1, 3), (0, 2), (0, 1), (1, 2), (2, 3), (0, 3)]
    assert sc[1] == float(np.float32(0.9))  # row 0's score, not row 2's
    got_p, got_s = nb.pairs_from_topk(torch.from_numpy(values), torch.from_numpy(indices), 10)
    assert [tuple(p) for p in got_p.tolist()] == pairs
    assert got_s.tolist() == [float(np.float32(s)) for s in sc]
    got_p, got_s = nb.pairs_from_topk(torch.from_numpy(values), torch.from_numpy(indices), 2)
    assert [tuple(p) for p in got_p.tolist()] == pairs[:2]
    # equal scores: (i asc, j asc)
    values = np.full((4, 3), 0.5, np.float32)
    indices = np.asarray([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], np.int32)
    pairs, _ = ref.pairs_from_topk(values, indices, 16)
    assert pairs == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert [tuple(p) for p in nb.pairs_from_topk(torch.from_numpy(values), torch.from_numpy(indices), 16)[0].tolist()] == pairs


def test_cluster_purity():
    labels = np.asarray([0, 0, 0, 1, 1, 2, 2, 2, 2])
    classes = np.asarray([5, 5, 1, 1, 1, 0, 3, 3, 0])
    assert ref.cluster_purity(labels, classes) == pytest.approx(6 / 9)
    assert nb.cluster_purity(torch.from_numpy(labels), torch.from_numpy(classes)) == pytest.approx(6 / 9)
    assert nb.cluster_purity(labels, labels) == 1.0
    with pytest.raises(ValueError, match="cluster_purity"):
        nb.cluster_purity(labels, classes[:-1])


def test_recall_at_k():
    indices = np.asarray([[0, 5, 6], [3, 1, 0], [7, 8, 9]])
    assert ref.recall_at_k(indices, np.arange(3), (1, 2, 3)) == {1: 1 / 3, 2: 2 / 3, 3: 2 / 3}
    assert nb.hits_at(torch.from_numpy(indices), torch.arange(3), (1, 2, 3)) == ref.recall_at_k(indices, np.arange(3), (1, 2, 3))


def test_the_kmeans_input_separates_far_beyond_fp32_rounding():
    """The precondition of the GPU k-means test: in every round of the restatement the smallest gap between a point's best and second
    best centre exceeds 4 * 768 * 2^-24 * max(|x|^2, |c|^2), so no fp32 rounding of a score can change a label."""
    X, init, planted = ref.kmeans_input()
    assert X.shape == (640, ref.D) and X.dtype == np.float32 and init.shape == (8,)
    assert [int(planted[i]) for i in init] == list(range(8))
    rounds, centers = ref.kmeans(X, init, 50)
    for r in rounds:
        bound = ref.kmeans_margin_bound(X, r["centers"])
        assert r["margin"] > bound, (r["margin"], bound)
        assert r["margin"] >= 1000 and bound < 0.2
    assert np.array_equal(rounds[0]["labels"], planted)  # recovered in one round
    assert len(rounds) == 2 and np.array_equal(rounds[1]["labels"], planted)
    assert rounds[1]["inertia"] < rounds[0]["inertia"]
    want, _ = ref.group_mean(X, np.arange(0, 641, 80), np.argsort(planted, kind="stable"))
    assert np.array_equal(centers, want)


def test_draw_init_is_philox_and_distinct():
    a = nb.draw_init(100, 18, 7)
    assert len(set(a.tolist())) == 18 and a.min() >= 0 and a.max() < 100
    assert np.array_equal(a, np.random.Generator(np.random.Philox(7)).choice(100, size=18, replace=False))
