"""A character n-gram language model over the decoder's own ids, for shallow fusion into beam search (csrc/ngram.hip).

The rule is stated in include/loco_asr.h: predicted symbols are the decoder ids 0 .. V - 1 (2 is the model's </s>), contexts may open with
BOS = V (the model's <s>, the start token at index 0 of a row), a backoff chain of at most ``order`` <= 8 symbols in float64 natural
logarithms.  It is this project's own rule, pinned by tests/ngram_ref.py; it is NOT validated against KenLM/SRILM binaries.

``NgramLM.train`` estimates interpolated Witten-Bell probabilities and writes them in backoff form; ``from_arpa`` / ``to_arpa`` read and
write ARPA files whose words are decimal ids plus ``<s>`` and ``</s>``.  Scoring runs on the device or not at all: ``.to(device)`` builds
the hash table there (loco_ngram_create), ``next_logprobs`` and ``token_logprobs`` are loco_op_ngram_logprobs / loco_op_ngram_score.

    python -m loco-asr_amd.ngram --ids FILE --order 6 --vocab 81 --out lm.arpa

trains on ``utt_id id id ...`` lines (the format ``transcribe --ref-ids`` reads; <s>, </s> and <pad> are dropped).
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
from collections import defaultdict
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_ORDER, MAX_VOCAB, MAX_GRAMS = 8, 127, 1 << 26
EOS_ID = 2
LN10 = math.log(10.0)
_BOS_LOG10 = -99.0  # ARPA's conventional log10 P(<s>); the unigram <s> is a context only and is never predicted


def _check_limits(order, vocab):
    if not 1 <= int(order) <= MAX_ORDER:
        raise ValueError(f"order = {order} is outside 1 .. {MAX_ORDER}")
    if not 3 <= int(vocab) <= MAX_VOCAB:
        raise ValueError(f"vocab = {vocab} is outside 3 .. {MAX_VOCAB}")


class NgramLM:
    """A backoff model as four host arrays -- ``lengths`` i32 [n], ``symbols`` i32 [n, 8] (oldest first, the predicted symbol last),
    ``logp`` and ``backoff`` f64 [n] -- and, after ``.to(device)``, the table on the device."""

    def __init__(self, order: int, vocab: int, lengths, symbols, logp, backoff):
        _check_limits(order, vocab)
        self.order, self.vocab = int(order), int(vocab)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        self.symbols = np.ascontiguousarray(symbols, dtype=np.int32).reshape(-1, MAX_ORDER)
        self.logp = np.ascontiguousarray(logp, dtype=np.float64)
        self.backoff = np.ascontiguousarray(backoff, dtype=np.float64)
        n = self.lengths.shape[0]
        if not (self.symbols.shape[0] == self.logp.shape[0] == self.backoff.shape[0] == n):
            raise ValueError("lengths, symbols, logp and backoff must describe the same grams")
        if not 1 <= n <= MAX_GRAMS:
            raise ValueError(f"{n} grams is outside 1 .. 2^26")
        self._handle, self.device = None, None

    def __len__(self):
        return int(self.lengths.shape[0])

    def grams(self):
        """{gram (tuple of symbols): (logp, backoff)}, for inspection and tests."""
        return {tuple(self.symbols[i, :self.lengths[i]].tolist()): (float(self.logp[i]), float(self.backoff[i])) for i in range(len(self))}

    # ---- estimation -------------------------------------------------------------------------------------------------------------
    @classmethod
    def train(cls, seqs, order: int, vocab: int) -> "NgramLM":
        """Interpolated Witten-Bell over id sequences without specials: every sequence is read as <s> ids </s>, grams start at <s> at
        the earliest.  P_j(w|h) = (c(hw) + T(h) P_{j-1}(w|h')) / (c(h) + T(h)) with T(h) the distinct successors of h and P_0 = 1/V,
        written in backoff form: logp of every seen gram (and of every id's unigram), bo(h) = T(h) / (c(h) + T(h))."""
        _check_limits(order, vocab)
        V, BOS = int(vocab), int(vocab)
        levels = [defaultdict(int) for _ in range(order)]  # levels[j][key]: grams of j + 1 symbols, key = symbols in base V + 1
        B = V + 1
        for seq in seqs:
            ids = [int(t) for t in seq]
            if any(t < 0 or t >= V for t in ids):
                raise ValueError(f"a training id is outside 0 .. {V - 1}")
            s = [BOS] + ids + [EOS_ID]
            for i in range(1, len(s)):
                key, scale = 0, 1
                for j in range(min(order, i + 1)):  # the gram s[i - j .. i]: the older symbol takes the higher digit
                    key += s[i - j] * scale
                    scale *= B
                    levels[j][key] += 1
        if not levels[0]:
            raise ValueError("train: no sequences")
        # per level: c(h) and T(h) of every context h, the gram without its last symbol (the low digit)
        lengths, symbols, logp, backoff = [], [], [], []
        ctx_stats = []
        for j in range(order):
            c, t = defaultdict(int), defaultdict(int)
            for key, n in levels[j].items():
                c[key // B] += n
                t[key // B] += 1
            ctx_stats.append((c, t))
        probs = []

        def lower(j, key):
            """P_{j}(w | h') for the gram of level j (j + 1 symbols) given by key, seen or not; level -1 is uniform"""
            if j < 0:
                return 1.0 / V
            got = probs[j].get(key)
            if got is not None:
                return got
            c, t = ctx_stats[j]
            h = key // B
            below = lower(j - 1, key % (B ** j))
            if h not in c:
                return below
            return (t[h] * below) / (c[h] + t[h])

        for j in range(order):
            c, t = ctx_stats[j]
            level = {}
            keys = set(levels[j])
            if j == 0:
                keys |= set(range(V))
            for key in keys:
                h = key // B
                level[key] = (levels[j].get(key, 0) + t[h] * lower(j - 1, key % (B ** j))) / (c[h] + t[h])
            probs.append(level)
        for j in range(order):
            nxt = ctx_stats[j + 1] if j + 1 < order else None
            for key in sorted(probs[j]):
                syms, k = [], key
                for _ in range(j + 1):
                    syms.append(k % B)
                    k //= B
                syms.reverse()
                lengths.append(j + 1)
                symbols.append(syms + [0] * (MAX_ORDER - j - 1))
                logp.append(math.log(probs[j][key]))
                bo = 0.0
                if nxt is not None and key in nxt[0]:
                    bo = math.log(nxt[1][key] / (nxt[0][key] + nxt[1][key]))
                backoff.append(bo)
        # the context <s>: a unigram that is never predicted
        c, t = ctx_stats[1] if order > 1 else ({}, {})
        lengths.append(1)
        symbols.append([BOS] + [0] * (MAX_ORDER - 1))
        logp.append(_BOS_LOG10 * LN10)
        backoff.append(math.log(t[BOS] / (c[BOS] + t[BOS])) if BOS in c else 0.0)
        return cls(order, V, lengths, symbols, logp, backoff)

    # ---- ARPA ---------------------------------------------------------------------------------------------------------------------
    def _word(self, sym: int) -> str:
        return "<s>" if sym == self.vocab else "</s>" if sym == EOS_ID else str(sym)

    def to_arpa(self, path) -> None:
        """Writes log10 values as %.17g; words are decimal ids, ``<s>`` for BOS and ``</s>`` for id 2.  A backoff of 0 is left out."""
        by_len = defaultdict(list)
        for i in range(len(self)):
            by_len[int(self.lengths[i])].append(i)
        with open(path, "w", encoding="utf-8") as f:
            f.write("\\data\\\n")
            for n in sorted(by_len):
                f.write(f"ngram {n}={len(by_len[n])}\n")
            for n in sorted(by_len):
                f.write(f"\n\\{n}-grams:\n")
                for i in by_len[n]:
                    words = " ".join(self._word(int(s)) for s in self.symbols[i, :n])
                    tail = "" if self.backoff[i] == 0.0 else "\t%.17g" % (self.backoff[i] / LN10)
                    f.write("%.17g\t%s%s\n" % (self.logp[i] / LN10, words, tail))
            f.write("\n\\end\\\n")

    @classmethod
    def from_arpa(cls, path, vocab: int) -> "NgramLM":
        """Reads an ARPA file over the words ``0`` .. ``vocab - 1`` (decimal ids; id 2 is written ``</s>``), ``<s>`` and ``</s>``.
        ``<unk>`` is read only as the value given to ids that lack a unigram; without it a missing unigram is an error, as is the word
        ``2`` (it would be a second </s>).  log10 becomes ln by one float64 multiply."""
        V = int(vocab)
        lengths, symbols, logp, backoff = [], [], [], []
        section, order, unk, seen1 = 0, 0, None, set()
        with open(path, encoding="utf-8") as f:
            for no, raw in enumerate(f, 1):
                line = raw.strip()
                if not line or line == "\\data\\" or line.startswith("ngram "):
                    continue
                if line == "\\end\\":
                    break
                if line.startswith("\\"):
                    if not line.endswith("-grams:"):
                        raise ValueError(f"{path}:{no}: unknown section {line!r}")
                    section = int(line[1:line.index("-")])
                    if not 1 <= section <= MAX_ORDER:
                        raise ValueError(f"{path}:{no}: order {section} is outside 1 .. {MAX_ORDER}")
                    order = max(order, section)
                    continue
                parts = line.split()
                if section == 0 or len(parts) not in (section + 1, section + 2):
                    raise ValueError(f"{path}:{no}: not 'log10p word ... [log10bo]' with {section} words")
                words = parts[1:1 + section]
                if words == ["<unk>"]:
                    unk = float(parts[0]) * LN10
                    continue
                syms = []
                for w in words:
                    if w == "<s>":
                        syms.append(V)
                    elif w == "</s>":
                        syms.append(EOS_ID)
                    elif w == str(EOS_ID):
                        raise ValueError(f"{path}:{no}: the word '{EOS_ID}' beside </s>: id {EOS_ID} is written </s>")
                    elif w.isdigit() and int(w) < V:
                        syms.append(int(w))
                    else:
                        raise ValueError(f"{path}:{no}: word {w!r} is not an id below {V}, <s> or </s>")
                if section == 1:
                    seen1.add(syms[0])
                lengths.append(section)
                symbols.append(syms + [0] * (MAX_ORDER - section))
                logp.append(float(parts[0]) * LN10)
                backoff.append(float(parts[section + 1]) * LN10 if len(parts) == section + 2 else 0.0)
        for w in range(V):
            if w not in seen1:
                if unk is None:
                    raise ValueError(f"{path}: id {w} has no unigram and the file has no <unk> entry")
                lengths.append(1)
                symbols.append([w] + [0] * (MAX_ORDER - 1))
                logp.append(unk)
                backoff.append(0.0)
        if order == 0:
            raise ValueError(f"{path}: no n-gram section")
        return cls(order, V, lengths, symbols, logp, backoff)

    # ---- the device -----------------------------------------------------------------------------------------------------------------
    def to(self, device) -> "NgramLM":
        """Builds the table on ``device`` (loco_ngram_create refuses a malformed model by name); returns self."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("NgramLM has no CPU path: the table is looked up by csrc/ngram.hip")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._handle is not None and self.device == device:
            return self
        if self._handle is not None:  # a decoder pool that fused this model holds the table, not a copy of it
            raise RuntimeError(f"NgramLM: the table is on {self.device}; it does not move to {device} (close() it once no pool uses it, "
                               "or build another NgramLM)")
        lib = _lib.load()
        out = C.c_void_p()
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        with torch.cuda.device(device):
            _lib.check(lib.loco_ngram_create(self.vocab, self.order, len(self), p(self.lengths), p(self.symbols), p(self.logp), p(self.backoff),
                                             C.byref(out)), "loco_ngram_create")
        self._handle, self.device, self._lib = out, device, lib
        return self

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self._lib.loco_ngram_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    @property
    def handle(self):
        if self._handle is None:
            raise RuntimeError("NgramLM: call .to(device) first; there is no CPU path")
        return self._handle

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def next_logprobs(self, rows) -> torch.Tensor:
        """float64 [R, vocab] on the device: log P(w | row) for every next id w; a row holds the tokens so far, index 0 the start token."""
        handle = self.handle
        rows = [[int(t) for t in r] for r in rows]
        if not rows or any(not r for r in rows):
            raise ValueError("next_logprobs: every row holds at least its start token")
        S = max(len(r) for r in rows)
        tok = torch.zeros((len(rows), S), dtype=torch.int32)
        for i, r in enumerate(rows):
            tok[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
        cur = torch.tensor([len(r) for r in rows], dtype=torch.int32)
        with torch.cuda.device(self.device):
            tok, cur = tok.to(self.device), cur.to(self.device)
            out = torch.empty((len(rows), self.vocab), dtype=torch.float64, device=self.device)
            _lib.check(self._lib.loco_op_ngram_logprobs(handle, tok.data_ptr(), S, S, cur.data_ptr(), len(rows), out.data_ptr(), self._stream()),
                       "loco_op_ngram_logprobs")
        return out

    def token_logprobs(self, seqs) -> List[torch.Tensor]:
        """Per sequence (ids from the start token on, as the decoder returns them) float64 [len - 1] on the host: log P of every token
        after the first given the tokens before it.  One launch for all of ``seqs``."""
        handle = self.handle
        seqs = [torch.as_tensor(s).reshape(-1).to(torch.int32).cpu() for s in seqs]
        if not seqs:
            return []
        if any(int(s.shape[0]) < 1 for s in seqs):
            raise ValueError("token_logprobs: every sequence holds at least its start token")
        lens = [int(s.shape[0]) for s in seqs]
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        total = int(sum(lens))
        with torch.cuda.device(self.device):
            flat = torch.cat(seqs).to(self.device)
            st, ln = torch.from_numpy(starts).to(self.device), torch.tensor(lens, dtype=torch.int32, device=self.device)
            out = torch.empty(total, dtype=torch.float64, device=self.device)
            _lib.check(self._lib.loco_op_ngram_score(handle, flat.data_ptr(), total, st.data_ptr(), ln.data_ptr(), len(seqs), out.data_ptr(),
                                                     self._stream()), "loco_op_ngram_score")
            host = out.cpu()
        return [host[a + 1:a + n].clone() for a, n in zip(starts.tolist(), lens)]

    def perplexity(self, seqs, start_token: int = EOS_ID) -> float:
        """exp(-sum log P / tokens) over id sequences without specials, each read as <s> ids </s> (the </s> counts, <s> does not)."""
        wrapped = [[start_token] + [int(t) for t in s] + [EOS_ID] for s in seqs]
        per = self.token_logprobs(wrapped)
        n = sum(int(p.shape[0]) for p in per)
        if n == 0:
            raise ValueError("perplexity: no tokens")
        return math.exp(-sum(float(p.sum()) for p in per) / n)


def read_id_lines(path) -> List[np.ndarray]:
    """``utt_id id id ...`` lines (what ``transcribe --ref-ids`` reads) as id sequences without <s>, </s> and <pad>."""
    from .metrics import strip_specials
    out = []
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            try:
                ids = [int(t) for t in parts[1:]]
            except ValueError:
                raise SystemExit(f"{path}:{no}: not 'utt_id id id ...'") from None
            out.append(strip_specials(ids))
    return out


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m loco-asr_amd.ngram", description="Train a character n-gram model over decoder ids (Witten-Bell).")
    ap.add_argument("--ids", required=True, metavar="FILE", help="'utt_id id id ...' lines, the format transcribe --ref-ids reads")
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--vocab", type=int, default=81)
    ap.add_argument("--out", required=True, metavar="FILE", help="the ARPA file to write")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    try:
        lm = NgramLM.train(read_id_lines(args.ids), args.order, args.vocab)
    except ValueError as e:
        raise SystemExit(f"--ids {args.ids}: {e}")
    lm.to_arpa(args.out)
    print(f"{args.out}: order {lm.order}, vocab {lm.vocab}, {len(lm)} grams")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
