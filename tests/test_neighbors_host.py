"""Host side of the neighbour module: every refusal happens before anything is launched and names its argument; the explore CLI's
argument surface; loco_topk_scratch_bytes.  No GPU."""
import importlib

import numpy as np
import pytest
import torch

nb = importlib.import_module("loco-asr_amd.neighbors")
explore = importlib.import_module("loco-asr_amd.explore")
_lib = importlib.import_module("loco-asr_amd._lib")
store_mod = importlib.import_module("loco-asr_amd.embedding_store")


def mat(rows, dim=768, dtype=torch.float32):
    return torch.zeros((rows, dim), dtype=dtype)


def test_cpu_tensors_are_refused_by_name():
    with pytest.raises(ValueError, match=r"queries: .*no CPU path"):
        nb.topk(mat(4), mat(9), k=2)
    with pytest.raises(ValueError, match=r"x: .*no CPU path"):
        nb.row_norm2(mat(4))
    with pytest.raises(ValueError, match=r"rows: .*no CPU path"):
        nb.group_mean(mat(4), torch.tensor([0, 4]))
    with pytest.raises(ValueError, match=r"vecs: .*no CPU path"):
        nb.mine_pairs(mat(4), top_k=2)
    with pytest.raises(ValueError, match=r"X: .*no CPU path"):
        nb.kmeans(mat(20), n_clusters=3)
    with pytest.raises(ValueError, match=r"queries: .*no CPU path"):
        nb.recall_at_k(mat(4), mat(4), ks=(1,))
    with pytest.raises(ValueError, match=r"queries: .*no CPU path"):
        nb.knn_classify(mat(9), np.zeros(9, np.int64), mat(4), k=3, n_classes=2)


def test_a_feature_dimension_other_than_768_is_refused():
    with pytest.raises(ValueError, match=r"queries: the feature dimension must be 768"):
        nb.topk(mat(4, 512), mat(9), k=2)
    with pytest.raises(ValueError, match=r"keys: the feature dimension must be 768"):
        nb.topk(mat(4), mat(9, 1024), k=2)
    with pytest.raises(ValueError, match=r"keys: the feature dimension must be 768"):
        nb.topk(mat(4), torch.zeros(768), k=2)
    with pytest.raises(ValueError, match=r"X: the feature dimension must be 768"):
        nb.kmeans(mat(20, 64), n_clusters=3)
    with pytest.raises(ValueError, match=r"vecs: the feature dimension must be 768"):
        nb.mine_pairs(mat(20, 767))


@pytest.mark.parametrize("k", [0, 17, -1, 2.5])
def test_k_outside_1_to_16_is_refused(k):
    with pytest.raises(ValueError, match=r"k = .* is outside 1 \.\. 16"):
        nb.topk(mat(4), mat(9), k=k)
    with pytest.raises(ValueError, match=r"top_k = .* is outside 1 \.\. 16"):
        nb.mine_pairs(mat(4), top_k=k)
    with pytest.raises(ValueError, match=r"ks entry = .* is outside 1 \.\. 16"):
        nb.recall_at_k(mat(4), mat(4), ks=(1, k))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16, torch.int32])
def test_a_dtype_other_than_fp32_is_refused(dtype):
    with pytest.raises(ValueError, match=r"queries: dtype .* is not torch.float32"):
        nb.topk(mat(4, dtype=dtype), mat(9), k=2)
    with pytest.raises(ValueError, match=r"keys: dtype .* is not torch.float32"):
        nb.topk(mat(4), mat(9, dtype=dtype), k=2)
    with pytest.raises(ValueError, match=r"X: dtype .* is not torch.float32"):
        nb.kmeans(mat(20, dtype=dtype), n_clusters=3)


def test_exclude_of_another_length_is_refused():
    with pytest.raises(ValueError, match=r"exclude: expected one key index per query \(4\)"):
        nb.topk(mat(4), mat(9), k=2, exclude=[0, 1, 2])
    with pytest.raises(ValueError, match=r"exclude: expected one key index per query \(4\)"):
        nb.topk(mat(4), mat(9), k=2, exclude=torch.zeros((4, 1), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"exclude: expected one key index per query \(9\)"):
        nb.knn_classify(mat(9), np.zeros(9, np.int64), mat(9), k=3, n_classes=2, exclude=np.arange(8))


def test_more_clusters_than_points_is_refused():
    with pytest.raises(ValueError, match=r"n_clusters = 21 exceeds the 20 points"):
        nb.kmeans(mat(20), n_clusters=21)
    with pytest.raises(ValueError, match=r"init: expected 3 integer row indices"):
        nb.kmeans(mat(20), n_clusters=3, init=[0, 1])
    with pytest.raises(ValueError, match=r"init: a row index outside 0 \.\. 19"):
        nb.kmeans(mat(20), n_clusters=3, init=[0, 1, 20])


def test_other_arguments_are_refused_by_name():
    with pytest.raises(ValueError, match=r"metric = 'euclid'"):
        nb.topk(mat(4), mat(9), k=2, metric="euclid")
    with pytest.raises(ValueError, match=r"labels: expected one class per row of train \(9\)"):
        nb.knn_classify(mat(9), np.zeros(8, np.int64), mat(4), k=3, n_classes=2)
    with pytest.raises(ValueError, match=r"labels: values outside 0 \.\. n_classes - 1"):
        nb.knn_classify(mat(9), np.full(9, 2), mat(4), k=3, n_classes=2)
    with pytest.raises(ValueError, match=r"partner: expected one key index per query \(4\)"):
        nb.recall_at_k(mat(4), mat(4), ks=(1,), partner=[0, 1])
    with pytest.raises(ValueError, match=r"offsets: expected int64"):
        nb.group_mean(mat(4), torch.tensor([0, 4], dtype=torch.int32))


def test_a_host_store_does_not_pool():
    store = store_mod.EmbeddingStore.from_arrays(["a", "b"], [np.ones((3, 768), np.float32), np.ones((2, 768), np.float32)],
                                                 [np.eye(101)[0], np.eye(101)[1]], device="cpu")
    with pytest.raises(ValueError, match=r"pooled: the store is on cpu; there is no CPU path"):
        store.pooled("average")
    with pytest.raises(ValueError, match=r"how = 'first'"):
        store.pooled("first")


def test_scratch_bytes():
    lib = _lib.load()
    assert lib.loco_topk_max_k() == 16 == nb.MAX_K
    f = lib.loco_topk_scratch_bytes
    for bad in [(0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, -1, 1), (5, 5, 0), (5, 5, 17), (5, 5, -1), (2 ** 31, 5, 1), (5, 2 ** 31, 1)]:
        assert f(*bad) == 0, bad
    for M, N, k in [(1, 1, 1), (1, 1024, 1), (1, 1025, 1), (300, 2049, 16), (131072, 131072, 10)]:
        assert f(M, N, k) == 8 * M * ((N + 1023) // 1024) * k
    assert f(2, 1024, 5) == 2 * f(1, 1024, 5) and f(1, 2048, 5) == 2 * f(1, 1024, 5) and f(1, 1024, 10) == 2 * f(1, 1024, 5)


def test_slabs_stay_under_the_cap_and_cover_every_query():
    assert nb.slab_rows(300, 2049, 16, 100 * 3 * 16 * 8) == 100
    assert nb.slab_rows(131072, 131072, 10, nb.SCRATCH_CAP) % 128 == 0
    rows = nb.slab_rows(131072, 131072, 10, nb.SCRATCH_CAP)
    assert rows * 128 * 10 * 8 <= nb.SCRATCH_CAP < (rows + 128) * 128 * 10 * 8
    assert nb.slab_rows(5, 10, 1, 1) == 1  # never below one query
    assert nb.slab_rows(40, 10, 1, 1 << 30) == 40


def test_cli_argument_surface():
    ap = explore.parser()
    a = ap.parse_args("--folder f --splits devel test --queries audio --keys text --k 1 5 10 --knn 10 --kmeans 18 --pairs 10 --metric cosine "
                      "--out report.json".split())
    assert (a.folder, a.splits, a.queries, a.keys, a.k, a.knn, a.kmeans, a.pairs, a.metric, a.out) == \
        ("f", ["devel", "test"], "audio", "text", [1, 5, 10], 10, 18, 10, "cosine", "report.json")
    d = ap.parse_args(["--folder", "f", "--out", "-"])
    assert (d.splits, d.queries, d.keys, d.k, d.knn, d.kmeans, d.pairs, d.metric) == (["devel"], "audio", "text", [1, 5, 10], 10, 0, 0, "cosine")
    for bad in (["--k", "17"], ["--k", "0"], ["--knn", "17"], ["--pairs", "17"], ["--metric", "euclid"], ["--queries", "text"], ["--kmeans", "-1"]):
        with pytest.raises(SystemExit):
            args = ap.parse_args(["--folder", "f", "--out", "-"] + bad)
            explore.check_args(args, ap)
    with pytest.raises(SystemExit):
        ap.parse_args(["--out", "-"])  # --folder is required


def test_ids_of_one_side_only_are_named_once_and_dropped():
    import io
    err = io.StringIO()
    ra, rb = explore.match_ids(["u1", "u2", "u3", "u5"], ["u3", "u9", "u1", "u7"], "audio", "text", err=err)
    assert (ra, rb) == ([0, 2], [2, 0])
    lines = err.getvalue().splitlines()
    assert lines == ["dropped 2 ids present in audio only: u2 u5", "dropped 2 ids present in text only: u9 u7"]
