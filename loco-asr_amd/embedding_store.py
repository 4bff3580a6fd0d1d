"""Device-resident ragged embedding store for training the intent head (``train_head.py --device-resident``).

The default training loop reads the reference's pickle folders through ``sink.EmbeddingsTargets`` and a ``DataLoader`` --
one file unpickled per utterance per epoch, padded on the host, copied from pageable memory.  SLURP's embeddings fit in HBM
many times over, so this store loads them ONCE: every clip's frames laid end to end in one ``rows [n_rows, 768]`` fp32
tensor, with ``offsets`` (int64, in rows) and ``lengths`` (int32) per clip and the targets as ``[n_items, 101]`` fp32.  A
batch is then only its index vector; the head's ragged kernels (``loco_head_*_ragged``) gather the clips by index and pool
them exactly as if ``pad_sequence`` had zero-padded them to the batch's longest clip.

    store = EmbeddingStore.from_folders("extracted/speecht5_base", "audio", ["train"], "cuda")
    idx, T_pad = store.batch([17, 3, 912])          # no device sync
    loss, logits = head.train_step_ragged(store, idx, T_pad)

Item order is that of ``ConcatDataset([EmbeddingsTargets(folder, modality, split) for split in splits])``, so the same
permutation yields the same batches as the default loop.  ``device="cpu"`` builds the store on the host (for tests; the head
itself has no CPU path).
"""
from __future__ import annotations

import os
import pickle
from concurrent.futures import ThreadPoolExecutor
from typing import Sequence

import numpy as np
import torch

D, NCLS = 768, 101
_STAGE_BYTES = 256 << 20  # host -> device copies go through pinned chunks of at most this size


def _read(path):
    with open(path, "rb") as fh:
        d = pickle.load(fh)
    return d["id"], np.asarray(d["embedding"], dtype=np.float32), np.asarray(d["target"])


class EmbeddingStore:
    """Ragged store: ``ids`` (list), ``lengths`` (host numpy int32), ``offsets_host`` (host numpy int64); on ``device``:
    ``rows`` [n_rows, 768] fp32, ``offsets`` int64, ``lengths_dev`` int32, ``targets`` [n_items, 101] fp32; ``nbytes``."""

    def __init__(self, ids, lengths: np.ndarray, rows: torch.Tensor, targets: torch.Tensor):
        self.ids = list(ids)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        self.offsets_host = np.zeros(len(self.lengths), dtype=np.int64)
        if len(self.lengths) > 1:
            np.cumsum(self.lengths[:-1], dtype=np.int64, out=self.offsets_host[1:])
        self.rows = rows
        self.targets = targets
        self.device = rows.device
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.lengths_dev = torch.from_numpy(self.lengths).to(self.device)

    def __len__(self):
        return len(self.ids)

    @property
    def n_rows(self) -> int:
        return int(self.rows.shape[0])

    @property
    def nbytes(self) -> int:
        """bytes the store occupies on its device: rows, targets, offsets and lengths"""
        return sum(t.numel() * t.element_size() for t in (self.rows, self.targets, self.offsets, self.lengths_dev))

    # ---- construction -----------------------------------------------------------------------------------------
    @staticmethod
    def _bytes_needed(n_rows, n_items):
        return n_rows * D * 4 + n_items * (NCLS * 4 + 8 + 4)

    @staticmethod
    def _check_fits(device, need):
        if device.type != "cuda":
            return
        free, total = torch.cuda.mem_get_info(device)
        if need > free:
            raise MemoryError(f"the embedding store needs {need} bytes ({need / 2**30:.2f} GiB) on {device}, but only {free} bytes "
                              f"({free / 2**30:.2f} GiB) of {total} are free")

    @classmethod
    def from_arrays(cls, ids: Sequence, embeddings: Sequence, targets: Sequence, device="cuda") -> "EmbeddingStore":
        """Build a store in-process from per-clip ``embeddings`` ([T_i, 768] arrays or tensors) and ``targets`` ([101] each),
        e.g. straight from extraction output."""
        device = torch.device(device)
        if not (len(ids) == len(embeddings) == len(targets)) or len(ids) == 0:
            raise ValueError(f"ids / embeddings / targets must be non-empty and of one length, got {len(ids)}, {len(embeddings)}, "
                             f"{len(targets)}")
        embs = [e.detach().cpu().float().numpy() if torch.is_tensor(e) else np.asarray(e, dtype=np.float32) for e in embeddings]
        for i, e in enumerate(embs):
            if e.ndim != 2 or e.shape[1] != D or e.shape[0] < 1:
                raise ValueError(f"embedding {i} ({ids[i]!r}) must be [frames >= 1, 768], got {e.shape}")
        tg = np.stack([t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in targets]).astype(np.float32)
        if tg.shape != (len(ids), NCLS):
            raise ValueError(f"targets must be [n, 101], got {tg.shape}")
        lengths = np.array([e.shape[0] for e in embs], dtype=np.int64)
        if lengths.max() > np.iinfo(np.int32).max:
            raise ValueError("a clip longer than 2^31 frames")
        n_rows = int(lengths.sum())
        cls._check_fits(device, cls._bytes_needed(n_rows, len(ids)))
        rows = cls._upload(embs, n_rows, device)
        return cls(ids, lengths.astype(np.int32), rows, torch.from_numpy(tg).to(device))

    @classmethod
    def from_folders(cls, folder: str, modality: str, splits: Sequence[str], device="cuda", workers: int = 8) -> "EmbeddingStore":
        """Read ``{folder}/{split}/{modality}/*.pickle`` for every split (the reference's format, sink.py) once, with a thread pool,
        in the item order of ``ConcatDataset([EmbeddingsTargets(folder, modality, s) for s in splits])``."""
        paths = []
        for split in splits:
            full = os.path.join(os.path.join(folder, split), modality)
            paths += [os.path.join(full, f) for f in sorted(f for f in os.listdir(full) if f.endswith(".pickle"))]
        if not paths:
            raise ValueError(f"no .pickle files under {folder}/{{{','.join(splits)}}}/{modality}")
        with ThreadPoolExecutor(max_workers=max(1, workers)) as ex:
            items = list(ex.map(_read, paths))
        ids = [it[0] for it in items]
        embs = [it[1] for it in items]
        targets = [it[2] for it in items]
        del items
        return cls.from_arrays(ids, embs, targets, device)

    @staticmethod
    def _upload(embs, n_rows, device):
        if device.type != "cuda":
            return torch.from_numpy(np.concatenate(embs, axis=0))
        rows = torch.empty(n_rows, D, dtype=torch.float32, device=device)
        stage_rows = max(max(e.shape[0] for e in embs), _STAGE_BYTES // (D * 4))
        stage = torch.empty(stage_rows, D, dtype=torch.float32, pin_memory=True)
        sv = stage.numpy()
        at, i = 0, 0
        while i < len(embs):
            n = 0
            while i < len(embs) and n + embs[i].shape[0] <= stage_rows:
                sv[n:n + embs[i].shape[0]] = embs[i]
                n += embs[i].shape[0]
                i += 1
            rows[at:at + n].copy_(stage[:n])  # synchronous: the staging buffer is refilled next
            at += n
        return rows

    # ---- pooling ----------------------------------------------------------------------------------------------
    def pooled(self, how: str = "average") -> torch.Tensor:
        """f32 [n_items, 768] on the device: the mean of each clip's stored frames -- padded frames included, as the notebooks'
        ``torch.mean(dim=1)`` includes them -- summed in double and rounded once (``loco_op_group_mean`` over the store's own
        offsets; nothing leaves the device).  There is no CPU path."""
        if how != "average":
            raise ValueError(f"how = {how!r}: only 'average' pooling is implemented")
        if self.device.type != "cuda":
            raise ValueError(f"pooled: the store is on {self.device}; there is no CPU path (loco_op_group_mean runs on the device)")
        from . import neighbors
        ends = torch.from_numpy(np.append(self.offsets_host, np.int64(self.n_rows))).to(self.device)
        out, _ = neighbors.group_mean(self.rows, ends)
        return out

    # ---- batches ----------------------------------------------------------------------------------------------
    def _check_indices(self, ind: np.ndarray):
        if ind.ndim != 1 or ind.size == 0:
            raise ValueError(f"a batch is a non-empty list of item indices, got shape {ind.shape}")
        if ind.min() < 0 or ind.max() >= len(self.ids):
            raise IndexError(f"batch index out of range [0, {len(self.ids)}): min {int(ind.min())}, max {int(ind.max())}")

    def batches(self, batch_list: Sequence[Sequence[int]]):
        """[(idx_dev int32 [B_i], T_pad_i)] for a list of batches, with ONE host-to-device copy for all of them (a pinned
        buffer, non-blocking: no device sync).  T_pad_i = the longest clip of batch i, from the host copy of the lengths."""
        arrs = [np.asarray(b, dtype=np.int64) for b in batch_list]
        for a in arrs:
            self._check_indices(a)
        flat = np.concatenate(arrs).astype(np.int32) if arrs else np.zeros(0, np.int32)
        host = torch.from_numpy(flat)
        if self.device.type == "cuda":
            host = host.pin_memory()
        dev = host.to(self.device, non_blocking=True)
        out, at = [], 0
        for a in arrs:
            out.append((dev[at:at + a.size], int(self.lengths[a].max())))
            at += a.size
        return out

    def batch(self, indices: Sequence[int]):
        """(idx_dev int32 [B], T_pad) for one batch; T_pad = max(lengths[indices]), what pad_sequence pads to."""
        return self.batches([indices])[0]

    def padded(self, indices: Sequence[int]):
        """(x [B, T_pad, 768], targets [B, 101]) of a batch, padded as collate_fn pads it (checks and tests)."""
        ind = np.asarray(indices, dtype=np.int64)
        self._check_indices(ind)
        T = int(self.lengths[ind].max())
        x = torch.zeros(len(ind), T, D, dtype=torch.float32, device=self.device)
        for b, i in enumerate(ind):
            o, n = int(self.offsets_host[i]), int(self.lengths[i])
            x[b, :n] = self.rows[o:o + n]
        return x, self.targets[torch.from_numpy(ind).to(self.device)]
