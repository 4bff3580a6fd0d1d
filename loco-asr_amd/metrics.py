"""Error rates and minimum-Bayes-risk selection: edit distance over symbol sequences on the device (csrc/edit_distance.hip).

The rule (include/loco_asr.h, "error rates") is integer and exact: MINIMUM COST, THEN MOST CORRECT SYMBOLS.  Among the alignments of
least edit distance the one with the fewest substitutions -- the most hits -- is counted, so (S, D, I, hits) is a property of the
pair of sequences and not of a traceback order.  ``cost = S + D + I``, and with it every error rate, is what sclite and Kaldi's
``compute-wer`` compute; the split into S / D / I is this project's own tie rule and can differ from theirs where alignments tie
(``ref = [1, 2]``, ``hyp = [2, 1]`` is one deletion and one insertion here, not two substitutions).

Symbols are int32: token ids as they are (``unit="token"``; for this character-level model a CER), words mapped to integers through
one dictionary per call (``words_of`` for id sequences split at a delimiter id, ``text_units`` for strings).  There is no host
fall-back: the dynamic programme runs in ``loco_op_edit_distance`` or not at all.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .decoder import DECODER_START_TOKEN_ID, EOS_TOKEN_ID, PAD_TOKEN_ID

# stripes of the launches a call is split into: pairs are bucketed by min(ref_len, hyp_len), the side the kernel stripes over a
# wave's lanes, so that one long pair does not size the LDS of a launch of short ones
_BUCKETS = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)


def max_len() -> int:
    """Symbols per side the kernel takes (``loco_edit_max_len``: 16384)."""
    return int(_lib.load().loco_edit_max_len())


@dataclass
class EditCounts:
    """Per pair, int32 device tensors [P]: substitutions, deletions, insertions, hits and the reference's length."""
    sub: torch.Tensor
    dele: torch.Tensor
    ins: torch.Tensor
    hits: torch.Tensor
    ref_len: torch.Tensor

    @property
    def cost(self) -> torch.Tensor:
        return self.sub + self.dele + self.ins


@dataclass
class ErrorRate:
    """Totals over ``pairs`` pairs, 0-d int64 device tensors; ``rate`` = (sub + dele + ins) / ref_len, 0-d float64 (nan without a
    reference symbol)."""
    rate: torch.Tensor
    sub: torch.Tensor
    dele: torch.Tensor
    ins: torch.Tensor
    ref_len: torch.Tensor
    pairs: int

    def kaldi_line(self, name: str = "WER") -> str:
        """``%WER 12.34 [ 123 / 997, 10 ins, 40 del, 73 sub ]`` as Kaldi's compute-wer prints it (one read-back)."""
        s, d, i, n = (int(v) for v in torch.stack([self.sub, self.dele, self.ins, self.ref_len]).cpu().tolist())
        return format_kaldi_line(name, s, d, i, n)


def format_kaldi_line(name: str, sub: int, dele: int, ins: int, ref_len: int) -> str:
    err = sub + dele + ins
    rate = 100.0 * err / ref_len if ref_len else float("nan")
    return f"%{name} {rate:.2f} [ {err} / {ref_len}, {ins} ins, {dele} del, {sub} sub ]"


@dataclass
class MbrResult:
    """``best`` int32 device tensor [U]: per list the first index of least risk; ``risk`` one float64 device tensor [N_u] per list."""
    best: torch.Tensor
    risk: List[torch.Tensor]


@dataclass
class MbrTranscripts:
    """What ``mbr_many`` returns: per utterance the chosen ``ids`` (host LongTensor), its index ``best`` (int) and the ``risk`` of every
    hypothesis (float64 device tensor [N]); ``hypotheses`` is ``sample_many``'s result, ``seed`` the seed it used, ``scores`` the
    hypotheses' per-token log-probabilities when asked for."""
    ids: list
    best: List[int]
    risk: List[torch.Tensor]
    hypotheses: list
    seed: Optional[int] = None
    scores: Optional[list] = None


# ---- symbols ----------------------------------------------------------------------------------------------------------------------
def _host_ids(ids) -> np.ndarray:
    if torch.is_tensor(ids):
        ids = ids.detach().cpu().numpy()
    arr = np.asarray(ids)
    if arr.size == 0:
        return np.zeros(0, dtype=np.int64)
    if arr.ndim != 1 or arr.dtype.kind not in "iu":
        raise ValueError(f"expected a 1-D sequence of integers, got shape {arr.shape} of {arr.dtype}")
    return arr.astype(np.int64)


def strip_specials(ids) -> np.ndarray:
    """A generated row without its leading start token, everything from its closing </s> on, and <pad>: int64 array (host)."""
    arr = _host_ids(ids)
    if arr.size and arr[0] == DECODER_START_TOKEN_ID:
        arr = arr[1:]
    ends = np.flatnonzero(arr == EOS_TOKEN_ID)
    if ends.size:
        arr = arr[:ends[0]]
    return arr[arr != PAD_TOKEN_ID]


def words_of(seqs, delimiter_id) -> List[np.ndarray]:
    """Id sequences -> word sequences: each is split at ``delimiter_id`` (empty words dropped) and every distinct word, a tuple of ids,
    gets an integer from ONE dictionary for the call, so equal words compare equal across the sequences of the call and only there.
    ``delimiter_id`` has no default: which id a checkpoint's word boundary carries is the caller's knowledge."""
    if delimiter_id is None:
        raise ValueError("words_of: delimiter_id is required (the id of the checkpoint's word-boundary token)")
    delimiter_id = int(delimiter_id)
    table: dict = {}
    out = []
    for seq in seqs:
        words, cur = [], []
        for t in _host_ids(seq).tolist() + [delimiter_id]:
            if t == delimiter_id:
                if cur:
                    words.append(table.setdefault(tuple(cur), len(table)))
                    cur = []
            else:
                cur.append(t)
        out.append(np.asarray(words, dtype=np.int32))
    return out


def text_units(lines: Sequence[str], unit: str) -> List[np.ndarray]:
    """Strings -> symbol sequences: ``"word"`` splits on whitespace and numbers the distinct words through one dictionary per call;
    ``"char"`` takes the code points."""
    if unit == "char":
        return [np.asarray([ord(ch) for ch in line], dtype=np.int32) for line in lines]
    if unit != "word":
        raise ValueError(f"unit = {unit!r} is not 'word' or 'char'")
    table: dict = {}
    return [np.asarray([table.setdefault(w, len(table)) for w in line.split()], dtype=np.int32) for line in lines]


# ---- the launch -------------------------------------------------------------------------------------------------------------------
def _device_of(seqs) -> torch.device:
    for s in seqs:
        if torch.is_tensor(s) and s.is_cuda:
            return s.device
    if not torch.cuda.is_available():
        raise RuntimeError("metrics: edit distances are computed on the device (loco_op_edit_distance); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _pack(seqs, device):
    """One int32 device buffer of all sequences and their (start, length) on the host.  Host sequences go up in one copy."""
    lens = np.asarray([int(s.numel()) if torch.is_tensor(s) else int(np.asarray(s).size) for s in seqs], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(seqs) else np.zeros(0, dtype=np.int64)
    if int(lens.sum()) > 2 ** 31 - 1:
        raise ValueError(f"{int(lens.sum())} symbols in one call exceed 2^31 - 1")
    if any(torch.is_tensor(s) and s.is_cuda for s in seqs):
        parts = []
        for k, s in enumerate(seqs):
            t = s if torch.is_tensor(s) else torch.from_numpy(_host_ids(s))
            if t.numel() and (t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool):
                raise ValueError(f"sequence {k}: expected a 1-D integer tensor, got shape {tuple(t.shape)} of {t.dtype}")
            parts.append(t.reshape(-1).to(device=device, dtype=torch.int64))
        wide = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=device)
        if wide.numel() and bool(((wide < -2 ** 31) | (wide > 2 ** 31 - 1)).any()):
            raise ValueError("a symbol does not fit int32")
        return wide.to(torch.int32), starts, lens
    host = np.concatenate([_host_ids(s) for s in seqs]) if len(seqs) else np.zeros(0, dtype=np.int64)
    if host.size and (host.min() < -2 ** 31 or host.max() > 2 ** 31 - 1):
        raise ValueError("a symbol does not fit int32")
    return torch.from_numpy(host.astype(np.int32)).to(device), starts, lens


def _run_pairs(symbols: torch.Tensor, spans: np.ndarray) -> torch.Tensor:
    """counts int32 [P, 4] (device) of spans int64 [P, 4] (host, already checked against the cap), one launch per bucket of
    min(ref_len, hyp_len)."""
    lib = _lib.load()
    device = symbols.device
    P = int(spans.shape[0])
    if P == 0:
        return torch.zeros((0, 4), dtype=torch.int32, device=device)
    stripe = np.minimum(spans[:, 1], spans[:, 3])
    bucket = np.searchsorted(np.asarray(_BUCKETS), stripe, side="left")
    order = np.argsort(bucket, kind="stable")
    sorted_spans = torch.from_numpy(np.ascontiguousarray(spans[order]).astype(np.int32)).to(device)
    counts = torch.empty((P, 4), dtype=torch.int32, device=device)
    if symbols.numel() == 0:  # only empty sequences: the pointer must still be one
        symbols = torch.zeros(1, dtype=torch.int32, device=device)
        n_symbols = 0
    else:
        n_symbols = int(symbols.numel())
    edges = np.searchsorted(bucket[order], np.arange(len(_BUCKETS) + 1), side="left")
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        for b, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            if hi > lo:
                _lib.check(lib.loco_op_edit_distance(symbols.data_ptr(), n_symbols, sorted_spans[lo:hi].data_ptr(), int(hi - lo), _BUCKETS[b],
                                                     counts[lo:hi].data_ptr(), stream), "loco_op_edit_distance")
    inverse = np.empty(P, dtype=np.int64)
    inverse[order] = np.arange(P)
    return counts.index_select(0, torch.from_numpy(inverse).to(device))


def _check_cap(lens, what):
    cap = max_len()
    over = np.flatnonzero(lens > cap)
    if over.size:
        k = int(over[0])
        raise ValueError(f"{what} {k}: {int(lens[k])} symbols exceed the {cap} a side may hold (loco_edit_max_len)")


def edit_counts(refs, hyps) -> EditCounts:
    """(S, D, I, hits) of every pair (refs[p], hyps[p]): equal-length lists of 1-D integer tensors or arrays, on the host or the
    device.  All sequences are packed into one symbol buffer and one spans array and compared on the device, one wave per pair;
    pairs are bucketed by length, one launch per bucket.  A sequence above ``max_len()`` symbols raises ValueError naming the pair
    before anything is launched."""
    refs, hyps = list(refs), list(hyps)
    if len(refs) != len(hyps):
        raise ValueError(f"edit_counts: {len(refs)} references for {len(hyps)} hypotheses")
    device = _device_of(refs + hyps)
    P = len(refs)
    lens = np.asarray([int(s.numel()) if torch.is_tensor(s) else int(np.asarray(s).size) for s in refs + hyps], dtype=np.int64)
    cap = max_len()
    over = np.flatnonzero(np.maximum(lens[:P], lens[P:]) > cap)
    if over.size:
        p = int(over[0])
        raise ValueError(f"edit_counts: pair {p}: a reference of {int(lens[p])} and a hypothesis of {int(lens[P + p])} symbols exceed the "
                         f"{cap} a side may hold (loco_edit_max_len)")
    symbols, starts, lens = _pack(refs + hyps, device)
    spans = np.stack([starts[:P], lens[:P], starts[P:], lens[P:]], axis=1) if P else np.zeros((0, 4), dtype=np.int64)
    counts = _run_pairs(symbols, spans)
    ref_len = torch.from_numpy(lens[:P].astype(np.int32)).to(device)
    return EditCounts(sub=counts[:, 0], dele=counts[:, 1], ins=counts[:, 2], hits=counts[:, 3], ref_len=ref_len)


def count_table(refs, hyps, unit: Optional[str] = None) -> List[List[int]]:
    """The ``[sub, del, ins, ref_len]`` lists of ``edit_counts(refs, hyps)``, one entry per pair, on the host after ONE read-back.
    ``unit=None``: symbol sequences as ``edit_counts`` takes them; ``"word"`` / ``"char"``: strings, runs of whitespace as one blank,
    turned into symbols by one ``text_units`` call over both sides (one dictionary of words for the call)."""
    refs, hyps = list(refs), list(hyps)
    if unit is not None:
        units = text_units([" ".join(s.split()) for s in refs + hyps], unit)
        refs, hyps = units[:len(refs)], units[len(refs):]
    c = edit_counts(refs, hyps)
    return torch.stack([c.sub, c.dele, c.ins, c.ref_len]).cpu().tolist()


def _fold(counts: EditCounts, pairs: int) -> ErrorRate:
    tot = torch.stack([counts.sub, counts.dele, counts.ins, counts.ref_len]).to(torch.int64).sum(dim=1)
    rate = (tot[0] + tot[1] + tot[2]).to(torch.float64) / tot[3].to(torch.float64)
    return ErrorRate(rate=rate, sub=tot[0], dele=tot[1], ins=tot[2], ref_len=tot[3], pairs=pairs)


def error_rate(refs, hyps) -> ErrorRate:
    """The corpus error rate of ``hyps`` against ``refs`` (``edit_counts``'s arguments): totals in int64 on the device,
    rate = (S + D + I) / N with N the references' symbols."""
    counts = edit_counts(refs, hyps)
    return _fold(counts, int(counts.sub.shape[0]))


# ---- n-best lists -----------------------------------------------------------------------------------------------------------------
def _units(seqs, unit, delimiter_id, what):
    if unit == "token":
        if delimiter_id is not None:
            raise ValueError(f"{what}: delimiter_id goes with unit='word'")
        return [strip_specials(s) for s in seqs]
    if unit == "word":
        if delimiter_id is None:
            raise ValueError(f"{what}: unit='word' needs delimiter_id, the id of the checkpoint's word-boundary token (there is no default)")
        return words_of([strip_specials(s) for s in seqs], delimiter_id)
    raise ValueError(f"{what}: unit = {unit!r} is not 'token' or 'word'")


def _list_weights(weights, scores, sizes):
    """float64 [total] on the host, or None for all ones."""
    if weights is None:
        if scores is not None:
            raise ValueError("mbr_select: scores= goes with weights='logprob'")
        return None
    if isinstance(weights, str):
        if weights != "logprob":
            raise ValueError(f"mbr_select: weights = {weights!r} is not None, 'logprob' or one list of numbers per list")
        if scores is None or len(scores) != len(sizes):
            raise ValueError("mbr_select: weights='logprob' needs scores=, one entry per hypothesis")
        flat = []
        for u, (per, n) in enumerate(zip(scores, sizes)):
            if len(per) != n:
                raise ValueError(f"mbr_select: list {u} has {n} hypotheses and {len(per)} scores")
            # a hypothesis's score: its sequence log-probability, or the per-token log-probabilities that sum to it
            s = np.asarray([float(torch.as_tensor(x).double().sum()) for x in per], dtype=np.float64)
            e = np.exp(s - s.max()) if n else s
            flat.append(e / e.sum() if n else e)
        w = np.concatenate(flat) if flat else np.zeros(0)
    else:
        if len(weights) != len(sizes) or any(len(per) != n for per, n in zip(weights, sizes)):
            raise ValueError("mbr_select: weights must hold one number per hypothesis")
        w = np.asarray([float(x) for per in weights for x in per], dtype=np.float64)
    if w.size and not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("mbr_select: weights must be finite and >= 0")
    first = 0
    for u, n in enumerate(sizes):
        if n and not w[first:first + n].sum() > 0:
            raise ValueError(f"mbr_select: the weights of list {u} sum to 0")
        first += n
    return w


def mbr_select(nbest, weights=None, unit: str = "token", delimiter_id: Optional[int] = None, scores=None) -> MbrResult:
    """Minimum-Bayes-risk selection: per n-best list the hypothesis of least expected edit distance to the list's others,
        risk[h] = sum over h' != h of w[h'] * cost(h, h') / sum over h' of w[h'].
    ``nbest[u][h]`` is as ``sample_many`` returns it (1-D ids, <s> ... </s>); the specials are stripped.  ``unit="token"`` compares
    ids, ``"word"`` the words between ``delimiter_id`` (required then).  ``weights=None`` weighs every hypothesis 1 -- Monte-Carlo
    MBR, the samples being draws from the model; ``weights="logprob"`` with ``scores=`` (per hypothesis its sequence log-probability
    or its per-token log-probabilities) uses the softmax of the sequence log-probabilities within the list; a list of lists gives
    the numbers themselves.  Ties go to the lowest index, so with ``greedy_first`` the greedy transcript wins them.  Every
    hypothesis is packed once; the N (N - 1) / 2 pairs of every list go through ``loco_op_edit_distance`` and one
    ``loco_op_nbest_risk`` launch."""
    nbest = [list(per) for per in nbest]
    sizes = [len(per) for per in nbest]
    if any(n < 1 for n in sizes):
        raise ValueError("mbr_select: every list needs at least one hypothesis")
    w = _list_weights(weights, scores, sizes)
    flat = [h for per in nbest for h in per]
    units = _units(flat, unit, delimiter_id, "mbr_select")
    lens = np.asarray([len(s) for s in units], dtype=np.int64)
    _check_cap(lens, "mbr_select: hypothesis")
    device = _device_of(flat)
    symbols, starts, lens = _pack(units, device)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if offsets[-1] > 2 ** 31 - 1:
        raise ValueError("mbr_select: too many hypotheses")
    left, right = [], []
    for u, n in enumerate(sizes):
        i, j = np.triu_indices(n, k=1)  # row-major (i < j)
        left.append(i + offsets[u])
        right.append(j + offsets[u])
    left = np.concatenate(left).astype(np.int64) if left else np.zeros(0, dtype=np.int64)
    right = np.concatenate(right).astype(np.int64) if right else np.zeros(0, dtype=np.int64)
    spans = np.stack([starts[left], lens[left], starts[right], lens[right]], axis=1)
    counts = _run_pairs(symbols, spans).contiguous()
    U, total = len(sizes), int(offsets[-1])
    if counts.shape[0] == 0:
        counts = torch.zeros((1, 4), dtype=torch.int32, device=device)
    risk = torch.empty(max(total, 1), dtype=torch.float64, device=device)
    best = torch.empty(max(U, 1), dtype=torch.int32, device=device)
    offs = torch.from_numpy(offsets.astype(np.int32)).to(device)
    wdev = None if w is None else torch.from_numpy(w).to(device)
    if U:
        lib = _lib.load()
        with torch.cuda.device(device):
            _lib.check(lib.loco_op_nbest_risk(counts.data_ptr(), offs.data_ptr(), None if wdev is None else wdev.data_ptr(), U, risk.data_ptr(),
                                              best.data_ptr(), torch.cuda.current_stream(device).cuda_stream), "loco_op_nbest_risk")
    return MbrResult(best=best[:U], risk=list(torch.split(risk[:total], sizes)) if U else [])


def oracle_error_rate(refs, nbest) -> ErrorRate:
    """The error rate of the best hypothesis an n-best list holds: per utterance the first hypothesis of least cost against the
    reference, folded like ``error_rate`` -- the bound on what any rescoring of the list can reach.  ``refs[u]`` and ``nbest[u][h]``
    are symbol sequences as ``edit_counts`` takes them (strip specials first)."""
    refs, nbest = list(refs), [list(per) for per in nbest]
    if len(refs) != len(nbest):
        raise ValueError(f"oracle_error_rate: {len(refs)} references for {len(nbest)} lists")
    sizes = [len(per) for per in nbest]
    if any(n < 1 for n in sizes):
        raise ValueError("oracle_error_rate: every list needs at least one hypothesis")
    if not refs:
        return error_rate([], [])
    counts = edit_counts([r for r, n in zip(refs, sizes) for _ in range(n)], [h for per in nbest for h in per])
    device = counts.sub.device
    U, width = len(sizes), max(sizes)
    rows = torch.from_numpy(np.repeat(np.arange(U), sizes)).to(device)
    cols = torch.from_numpy(np.concatenate([np.arange(n) for n in sizes])).to(device)
    table = torch.full((U, width), 2 ** 31 - 1, dtype=torch.int64, device=device)
    table[rows, cols] = counts.cost.to(torch.int64)
    # the first index of least cost (a stable sort keeps equal costs in index order)
    pick = torch.sort(table, dim=1, stable=True).indices[:, 0] + torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]])).to(device)
    chosen = EditCounts(*(getattr(counts, f).index_select(0, pick) for f in ("sub", "dele", "ins", "hits", "ref_len")))
    return _fold(chosen, U)
