"""The device-resident embedding store (embedding_store.py) on the host: the same items, in the same order, as the default
training loop's ConcatDataset of EmbeddingsTargets, ragged offsets that agree with the lengths, batches whose T_pad is what
pad_sequence pads to, and refused out-of-range indices.  device="cpu" builds the store on the host; only the head refuses CPU."""
import importlib
import os

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import ConcatDataset

sink = importlib.import_module("loco-asr_amd.sink")
es = importlib.import_module("loco-asr_amd.embedding_store")
train_head = importlib.import_module("loco-asr_amd.train_head")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp("emb")
    rng = np.random.default_rng(7)
    for split, n in (("train", 23), ("train_synthetic", 9), ("devel", 11)):
        folder = root / split / "audio"
        os.makedirs(folder)
        for i in range(n):
            T = int(rng.choice([1, 2, 37, 127, 128, 129, 300]))
            tgt = np.zeros(101, dtype=np.int64)
            tgt[int(rng.integers(0, 101))] = 1
            # ids deliberately not in file-name order within a split: the store must follow the sorted FILE names
            sink.write_one(str(folder), f"{split[:2]}{(i * 7) % n:03d}", rng.standard_normal((T, 768)).astype(np.float32), tgt)
    return str(root)


def test_from_folders_equals_the_concat_dataset_item_by_item(corpus):
    splits = ["train", "train_synthetic"]
    ds = ConcatDataset([sink.EmbeddingsTargets(corpus, "audio", s) for s in splits])
    st = es.EmbeddingStore.from_folders(corpus, "audio", splits, device="cpu", workers=4)
    assert len(st) == len(ds) == 32
    for i in range(len(ds)):
        sid, emb, tgt = ds[i]
        assert st.ids[i] == sid
        o, n = int(st.offsets_host[i]), int(st.lengths[i])
        assert n == emb.shape[0]
        assert torch.equal(st.rows[o:o + n], emb)
        assert torch.equal(st.targets[i], tgt.float())


def test_offsets_and_lengths_are_consistent(corpus):
    st = es.EmbeddingStore.from_folders(corpus, "audio", ["train", "train_synthetic", "devel"], device="cpu")
    assert st.lengths.dtype == np.int32 and st.offsets_host.dtype == np.int64
    assert st.offsets.dtype == torch.int64 and st.lengths_dev.dtype == torch.int32
    assert st.offsets_host[0] == 0
    assert np.array_equal(st.offsets_host[1:], np.cumsum(st.lengths[:-1].astype(np.int64)))
    assert st.offsets_host[-1] + st.lengths[-1] == st.n_rows == st.rows.shape[0]
    assert np.array_equal(st.offsets.numpy(), st.offsets_host) and np.array_equal(st.lengths_dev.numpy(), st.lengths)
    assert tuple(st.targets.shape) == (len(st), 101) and st.targets.dtype == torch.float32


def test_nbytes(corpus):
    st = es.EmbeddingStore.from_folders(corpus, "audio", ["devel"], device="cpu")
    n = len(st)
    assert st.nbytes == st.n_rows * 768 * 4 + n * 101 * 4 + n * 8 + n * 4
    assert st.nbytes == es.EmbeddingStore._bytes_needed(st.n_rows, n)


def test_batch_T_pad_is_what_pad_sequence_pads_to(corpus):
    splits = ["train", "train_synthetic"]
    ds = ConcatDataset([sink.EmbeddingsTargets(corpus, "audio", s) for s in splits])
    st = es.EmbeddingStore.from_folders(corpus, "audio", splits, device="cpu")
    for batch in ([0], [3, 3, 1], [31, 0, 17, 5, 9], list(range(32))[::-1]):
        idx, T_pad = st.batch(batch)
        ref = pad_sequence([ds[i][1] for i in batch], batch_first=True)
        assert T_pad == ref.shape[1]
        assert idx.dtype == torch.int32 and idx.tolist() == batch
        x, t = st.padded(batch)
        assert torch.equal(x, ref)
        assert torch.equal(t, torch.stack([ds[i][2] for i in batch]).float())


def test_out_of_range_and_empty_batches_are_refused(corpus):
    st = es.EmbeddingStore.from_folders(corpus, "audio", ["devel"], device="cpu")
    with pytest.raises(IndexError):
        st.batch([0, len(st)])
    with pytest.raises(IndexError):
        st.batch([-1])
    with pytest.raises(ValueError):
        st.batch([])
    with pytest.raises(IndexError):
        st.batches([[0, 1], [2, 99]])


def test_epoch_batches_index_the_same_items_in_both_paths(corpus):
    """The default loop's DataLoader(batch_sampler=epoch_batches(...)) and the store's batches over the same index lists: the same
    ids, the same padded tensors, the same targets -- for two consecutive epochs of one seeded generator, at W = 1 and for rank 1 of 3."""
    splits = ["train", "train_synthetic"]
    ds = ConcatDataset([sink.EmbeddingsTargets(corpus, "audio", s) for s in splits])
    st = es.EmbeddingStore.from_folders(corpus, "audio", splits, device="cpu")
    for world, rank in ((1, 0), (3, 1)):
        g1, g2 = torch.Generator().manual_seed(0), torch.Generator().manual_seed(0)
        for _ in range(2):
            ids_a, mine_a = train_head.epoch_batches(len(ds), 16 if world == 1 else 4, world, rank, g1)
            ids_b, mine_b = train_head.epoch_batches(len(ds), 16 if world == 1 else 4, world, rank, g2)
            assert ids_a == ids_b and mine_a == mine_b
            loader = torch.utils.data.DataLoader(ds, batch_sampler=mine_a, collate_fn=train_head.collate_fn)
            for (sids, data, target), (idx, T_pad), lst in zip(loader, st.batches(mine_b), mine_b):
                assert list(sids) == [st.ids[i] for i in idx.tolist()]
                assert data.shape[1] == T_pad
                x, t = st.padded(lst)
                assert torch.equal(x, data) and torch.equal(t, target.float())


def test_from_arrays_matches_from_folders(corpus):
    a = es.EmbeddingStore.from_folders(corpus, "audio", ["devel"], device="cpu")
    ds = sink.EmbeddingsTargets(corpus, "audio", "devel")
    items = [ds[i] for i in range(len(ds))]
    b = es.EmbeddingStore.from_arrays([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], device="cpu")
    assert a.ids == b.ids and np.array_equal(a.lengths, b.lengths)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.targets, b.targets)
    with pytest.raises(ValueError):
        es.EmbeddingStore.from_arrays(["x"], [np.zeros((3, 512), np.float32)], [np.zeros(101)], device="cpu")
    with pytest.raises(ValueError):
        es.EmbeddingStore.from_arrays([], [], [], device="cpu")


def test_device_resident_flag_is_documented():
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        train_head.main(["--help"])
    text = " ".join(buf.getvalue().split()).lower()
    assert "--device-resident" in text and "every rank holds the whole train and validation store" in text
