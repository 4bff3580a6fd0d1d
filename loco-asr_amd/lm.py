"""GPT-2 language-model scorer on the MI355X: token negative log-likelihoods and per-recording perplexity.

The counterpart of the reference's ``lms/src/eval_ppl_with_pretrained_lm.py``: ``GPT2LMHeadModelMI355X`` holds HF's ``GPT2LMHeadModel``
weights ("gpt2": 12 x 768 x 12 heads) behind the C ABI's ``loco_lm_*`` entry points, and the two corpus walkers restate the reference's
two context modes (``indep``: every utterance alone; ``max_len``: a recording's whole left context, up to ``n_positions`` tokens).

Ids stay where they are: a call hands the library ONE 1-D int32 token buffer on the device plus per-sequence (start, length) pairs, so a
sliding window over a recording or a ragged batch of a corpus is a pair of small index arrays, never a ``[B, S]`` id matrix.  Only the
positions that are scored go through ``ln_f`` and the LM head, and the head never writes its ``[rows, 50257]`` logits
(``csrc/lm.hip``).  There is no CPU path.

The reference's edge behaviour in ``max_len`` mode is kept as it stands (``strict_reference=True``, the default):

* a recording of ``n`` >= ``n_positions`` tokens is walked by windows that start at offsets ``0 .. n - n_positions - 1``; the last of them
  ends at token ``n - 2``, so the recording's final token is never scored;
* a recording of exactly ``n_positions`` tokens therefore yields no window at all, and no perplexity.

``strict_reference=False`` adds the one missing window (offset ``n - n_positions``), which scores both.

A K/V cache (``model.new_cache``, ``append``, ``token_nll_given``, ``rescore``) scores continuations behind a context that is encoded
once, and ``score_carry`` walks a recording with such a cache: a third context mode that is NOT the reference's ``max_len`` but
HuggingFace's strided perplexity with utterance-aligned strides (``carry_plan``).
"""
from __future__ import annotations

import ctypes as C
import json
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

HIDDEN, HEADS = 768, 12
IGNORE_INDEX = -100
STATUS_CLEAN = 0x7F7F7F7F
_IGNORED_SUFFIXES = (".attn.bias", ".attn.masked_bias")


@dataclass
class CausalLMOutput:
    logits: "object" = None
    hidden_states: Optional[tuple] = None


def strip_key(key: str) -> str:
    return key[len("transformer."):] if key.startswith("transformer.") else key


def expected_keys(n_layer: int) -> List[str]:
    keys = ["wte.weight", "wpe.weight", "ln_f.weight", "ln_f.bias"]
    for l in range(n_layer):
        for leaf in ("ln_1", "ln_2", "attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"):
            keys += [f"h.{l}.{leaf}.weight", f"h.{l}.{leaf}.bias"]
    return keys


def config_from_state_dict(sd) -> dict:
    """n_layer / n_positions / vocab_size / n_embd read off a GPT2LMHeadModel (or GPT2Model) state dict."""
    keys = {strip_key(k): k for k in sd}
    if "wte.weight" not in keys or "wpe.weight" not in keys:
        raise KeyError("not a GPT-2 state dict: no (transformer.)wte.weight / wpe.weight")
    layers = {int(k.split(".")[1]) for k in keys if k.startswith("h.")}
    if not layers or layers != set(range(max(layers) + 1)):
        raise KeyError(f"GPT-2 state dict: block indices {sorted(layers)} are not 0 .. n_layer - 1")
    wte, wpe = sd[keys["wte.weight"]], sd[keys["wpe.weight"]]
    return {"n_layer": max(layers) + 1, "n_positions": int(wpe.shape[0]), "vocab_size": int(wte.shape[0]), "n_embd": int(wte.shape[1])}


class GPT2LMHeadModelMI355X:
    """HF's ``GPT2LMHeadModel`` for scoring: ``model(input_ids).logits`` (small calls) and ``model.token_nll`` (the product path)."""

    def __init__(self, n_layer: int = 12, n_positions: int = 1024, vocab_size: int = 50257, n_embd: int = HIDDEN, n_head: int = HEADS):
        self._lib = _lib.load()
        self._h = self._lib.loco_lm_create(n_layer, n_positions, vocab_size, n_embd, n_head)
        if not self._h:
            raise ValueError(self._lib.loco_last_error().decode(errors="replace"))
        self.n_layer, self.n_positions, self.vocab_size = n_layer, n_positions, vocab_size
        self._sd = None
        self._loaded = False
        self._ws = None
        self.device = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.loco_lm_destroy(h)

    # ---- construction ----
    @classmethod
    def from_state_dict(cls, sd, n_positions: Optional[int] = None, n_head: int = HEADS):
        cfg = config_from_state_dict(sd)
        if n_positions is not None and n_positions != cfg["n_positions"]:
            raise ValueError(f"n_positions = {n_positions} but wpe.weight has {cfg['n_positions']} rows")
        m = cls(cfg["n_layer"], cfg["n_positions"], cfg["vocab_size"], cfg["n_embd"], n_head)
        m.load_state_dict(sd)
        return m

    @classmethod
    def from_pretrained(cls, path: str):
        """A HuggingFace GPT-2 checkpoint directory on disk: ``config.json`` and ``model.safetensors`` or ``pytorch_model.bin``."""
        import torch
        from .checkpoint_map import _checkpoint_files
        cfg_path = os.path.join(path, "config.json")
        n_head = HEADS
        if os.path.exists(cfg_path):
            with open(cfg_path) as fh:
                cfg = json.load(fh)
            n_head = int(cfg.get("n_head", HEADS))
            if cfg.get("activation_function", "gelu_new") != "gelu_new":
                raise ValueError(f"{cfg_path}: activation_function = {cfg['activation_function']!r}; only gelu_new is implemented")
        sd = {}
        for f in _checkpoint_files(path):
            if f.endswith(".safetensors"):
                from safetensors import safe_open
                with safe_open(f, framework="pt", device="cpu") as sf:
                    for key in sf.keys():
                        sd[key] = sf.get_tensor(key)
            else:
                part = torch.load(f, map_location="cpu", weights_only=True)
                sd.update(part.get("state_dict", part) if isinstance(part, dict) else part)
        return cls.from_state_dict(sd, n_head=n_head)

    def load_state_dict(self, sd):
        """Check names and shapes now (no GPU needed); the tensors go to the device with ``.to("cuda")`` or the first call."""
        import torch
        kept: Dict[str, "torch.Tensor"] = {}
        head = None
        for k, v in sd.items():
            key = strip_key(k)
            t = torch.as_tensor(v)
            if key == "lm_head.weight":
                head = t
                continue
            if key.endswith(_IGNORED_SUFFIXES):
                continue
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            # a null data pointer: the library checks the name and the shape first and complains about the pointer last
            rc = self._lib.loco_lm_set_weight(self._h, k.encode(), None, shape, t.dim())
            msg = self._lib.loco_last_error().decode(errors="replace")
            if rc < 0 and "null data" not in msg:
                raise KeyError(msg)
            kept[key] = t
        missing = [k for k in expected_keys(self.n_layer) if k not in kept]
        if missing:
            raise KeyError(f"GPT-2 state dict: {len(missing)} tensors missing, e.g. {missing[:4]}")
        if head is not None and head is not sd.get("transformer.wte.weight", sd.get("wte.weight")):
            if head.shape != kept["wte.weight"].shape or not torch.equal(torch.as_tensor(head).cpu(), kept["wte.weight"].cpu()):
                raise ValueError("lm_head.weight differs from wte.weight: only the tied head of GPT2LMHeadModel is supported")
        self._sd, self._loaded = kept, False
        return self

    def to(self, device):
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("GPT2LMHeadModelMI355X has no CPU path: the model runs on a ROCm device only")
        self.device = device
        self._upload()
        return self

    def eval(self):
        return self

    def _upload(self):
        import torch
        if self._loaded:
            return
        if self._sd is None:
            raise RuntimeError("GPT2LMHeadModelMI355X: no weights loaded (from_pretrained / from_state_dict / load_state_dict)")
        with torch.cuda.device(self.device):
            for key, t in self._sd.items():
                d = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
                shape = (C.c_int64 * d.dim())(*d.shape)
                _lib.check(self._lib.loco_lm_set_weight(self._h, key.encode(), C.c_void_p(d.data_ptr()), shape, d.dim()), key)
            torch.cuda.synchronize(self.device)
            _lib.check(self._lib.loco_lm_finalize(self._h, self._stream()), "loco_lm_finalize")
        self._sd, self._loaded = None, True

    # ---- plumbing ----
    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, B, S, R):
        import torch
        need = self._lib.loco_lm_workspace_bytes(self._h, B, S, R)
        if need == 0:
            raise ValueError(f"B = {B}, S = {S}, R = {R}: outside the limits (1 <= S <= n_positions = {self.n_positions}, 1 <= B <= 65535)")
        if self._ws is None or self._ws.numel() < need or self._ws.device != self.device:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws, need

    def _need_cuda(self, t, what):
        import torch
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"GPT2LMHeadModelMI355X has no CPU path: {what} must be a tensor on a ROCm device")
        if self.device is None:
            self.device = t.device
        self._upload()

    def _check_status(self, ws, tokens):
        status = int(ws[:4].view(dtype=__import__("torch").int32).item())
        if status != STATUS_CLEAN:
            raise ValueError(f"token id {int(tokens[status].item())} at position {status} of the token buffer is outside [0, {self.vocab_size})")

    def _index(self, values):
        import torch
        return torch.as_tensor(np.asarray(values, dtype=np.int32), device=self.device)

    def nll_rows(self, tokens, starts: Sequence[int], lens: Sequence[int], S: int, rows: Sequence[int]):
        """The product call.  ``tokens``: 1-D int32 tensor on the device; sequence b is ``tokens[starts[b] : starts[b] + lens[b]]``;
        ``rows``: flat indices ``b * S + s`` of the positions to score, each against token ``s + 1`` of its sequence.  Returns the f32
        ``[len(rows)]`` NLLs on the device (0 where ``s + 1 >= lens[b]``)."""
        import torch
        self._need_cuda(tokens, "tokens")
        if tokens.dtype != torch.int32 or tokens.dim() != 1 or not tokens.is_contiguous():
            raise ValueError("tokens must be a contiguous 1-D int32 tensor")
        starts, lens, rows = np.asarray(starts, np.int64), np.asarray(lens, np.int64), np.asarray(rows, np.int64)
        B, R = len(starts), len(rows)
        if B < 1 or len(lens) != B or R < 1:
            raise ValueError("starts and lens must have the same non-zero length, rows at least one entry")
        if lens.min() < 0 or lens.max() > S or starts.min() < 0 or (starts + lens).max() > tokens.numel():
            raise ValueError(f"sequences must satisfy 0 <= len <= S = {S} and lie inside the {tokens.numel()}-token buffer")
        if rows.min() < 0 or rows.max() >= B * S:
            raise ValueError(f"rows must lie in [0, B * S = {B * S})")
        with torch.cuda.device(self.device):
            ws, need = self._workspace(B, S, R)
            d_starts, d_lens, d_rows = self._index(starts), self._index(lens), self._index(rows)
            out = torch.empty(R, dtype=torch.float32, device=self.device)
            p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            _lib.check(self._lib.loco_lm_nll(self._h, p(tokens), p(d_starts), p(d_lens), B, S, p(d_rows), R, p(out), p(ws), need, self._stream()),
                       "loco_lm_nll")
            self._check_status(ws, tokens)
        return out

    # ---- HF's contract ----
    def __call__(self, input_ids, output_hidden_states: bool = False, lengths=None):
        """``.logits`` f32 ``[B, S, V]`` (and the 13 ``hidden_states``): for tests and small calls -- the logits are materialised."""
        import torch
        self._need_cuda(input_ids, "input_ids")
        if input_ids.dim() != 2:
            raise ValueError("input_ids must be [B, S]")
        B, S = input_ids.shape
        tokens = input_ids.to(torch.int32).contiguous().view(-1)
        lens = np.full(B, S, np.int64) if lengths is None else np.asarray(lengths, np.int64)
        with torch.cuda.device(self.device):
            ws, need = self._workspace(B, S, 0)
            ldv = self._lib.loco_lm_vocab_stride(self._h)
            logits = torch.empty(B, S, ldv, dtype=torch.float32, device=self.device)
            hs = [torch.empty(B, S, HIDDEN, dtype=torch.float32, device=self.device) for _ in range(self.n_layer + 1)] if output_hidden_states else None
            hp = (C.c_void_p * (self.n_layer + 1))(*[t.data_ptr() for t in hs]) if hs else None
            d_starts, d_lens = self._index(np.arange(B) * S), self._index(lens)
            p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            _lib.check(self._lib.loco_lm_forward(self._h, p(tokens), p(d_starts), p(d_lens), B, S, hp, p(logits), p(ws), need, self._stream()),
                       "loco_lm_forward")
            self._check_status(ws, tokens)
        return CausalLMOutput(logits=logits[..., :self.vocab_size], hidden_states=tuple(hs) if hs else None)

    forward = __call__

    def token_nll(self, input_ids, lengths=None):
        """f32 ``[B, S - 1]``: entry (b, s) = -log P(input_ids[b, s + 1] | input_ids[b, :s + 1]); 0 from ``lengths[b] - 1`` on."""
        import torch
        self._need_cuda(input_ids, "input_ids")
        if input_ids.dim() != 2 or input_ids.shape[1] < 2:
            raise ValueError("input_ids must be [B, S] with S >= 2")
        B, S = input_ids.shape
        tokens = input_ids.to(torch.int32).contiguous().view(-1)
        lens = np.full(B, S, np.int64) if lengths is None else np.asarray(lengths, np.int64)
        rows = (np.arange(B)[:, None] * S + np.arange(S - 1)[None, :]).reshape(-1)
        return self.nll_rows(tokens, np.arange(B) * S, lens, S, rows).view(B, S - 1)

    def token_nll_ragged(self, seqs: Sequence, batch_size: int = 128) -> list:
        """One f32 ``[len - 1]`` tensor per 1-D id tensor of ``seqs`` (any lengths >= 2), in the order given.  The ids are laid end to
        end in one device buffer; batches of at most ``batch_size`` sequences are taken in order of length."""
        import torch
        if not len(seqs):
            return []
        for t in seqs:
            self._need_cuda(t, "every sequence")
            if t.dim() != 1 or t.numel() < 2:
                raise ValueError("every sequence must be 1-D with at least 2 tokens")
        lens = np.asarray([t.numel() for t in seqs], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)])
        tokens = torch.cat([t.to(torch.int32) for t in seqs]).contiguous()
        order = np.argsort(lens, kind="stable")
        out: list = [None] * len(seqs)
        for i in range(0, len(order), batch_size):
            idx = order[i:i + batch_size]
            S = int(lens[idx].max())
            rows = np.concatenate([b * S + np.arange(lens[j] - 1) for b, j in enumerate(idx)])
            nll = self.nll_rows(tokens, offs[idx], lens[idx], S, rows)
            for piece, j in zip(torch.split(nll, [int(lens[j] - 1) for j in idx]), idx):
                out[j] = piece
        return out

    # ---- cached context (csrc/lm_attention.hip) ----
    def new_cache(self, slots: int = 1, device=None) -> "LmCache":
        """``slots`` independent contexts (1 .. 64), each up to ``n_positions`` tokens of K/V in fp32 on the device."""
        import torch
        device = torch.device(device) if device is not None else (self.device or torch.device("cuda"))
        if device.type != "cuda":
            raise RuntimeError("GPT2LMHeadModelMI355X has no CPU path: a cache lives on a ROCm device only")
        if self.device is None:
            self.device = device
        self._upload()
        return LmCache(self, slots)

    def _ctx_step(self, cache: "LmCache", tokens, seqs: Sequence[Tuple[int, int, int, int]]):
        """One ``loco_lm_ctx_step``: ``seqs`` = (start, len, slot, flags) per sequence.  Returns the flat f32 NLLs of the scoring sequences
        (or None).  Host-side refusals (a full slot, two commits on one slot, ...) raise ValueError with the library's message."""
        import torch
        if cache.model is not self:
            raise ValueError("the cache belongs to another model")
        arr = np.ascontiguousarray(np.asarray(seqs, np.int32).reshape(-1, 4))
        if tokens.dtype != torch.int32 or tokens.dim() != 1 or not tokens.is_contiguous():
            raise ValueError("tokens must be a contiguous 1-D int32 tensor")
        if len(arr) and (arr[:, 0].min() < 0 or (arr[:, 0].astype(np.int64) + arr[:, 1].clip(min=0)).max() > tokens.numel()):
            raise ValueError(f"every sequence must lie inside the {tokens.numel()}-token buffer")
        N, rows = len(arr), int(arr[:, 1].clip(min=0).sum())
        R = int(arr[arr[:, 3] & 1 == 1, 1].clip(min=0).sum())
        with torch.cuda.device(self.device):
            need = self._lib.loco_lm_ctx_workspace_bytes(self._h, max(rows, N), N)
            if need and (self._ws is None or self._ws.numel() < need or self._ws.device != self.device):
                self._ws = None
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            ws = self._ws if self._ws is not None else torch.empty(256, dtype=torch.uint8, device=self.device)
            out = torch.empty(max(R, 1), dtype=torch.float32, device=self.device)
            p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            rc = self._lib.loco_lm_ctx_step(self._h, cache._h, p(tokens), arr.ctypes.data_as(C.POINTER(C.c_int32)), N, p(out), p(ws), ws.numel(),
                                            self._stream())
            if rc < 0:
                raise ValueError(self._lib.loco_last_error().decode(errors="replace"))
            self._check_status(ws, tokens)
        return out[:R] if R else None

    def _ids(self, ids, what):
        import torch
        self._need_cuda(ids, what)
        if ids.dim() != 1 or ids.numel() < 1:
            raise ValueError(f"{what} must be a 1-D tensor of at least one GPT-2 id")
        return ids.to(torch.int32).contiguous()

    def append(self, cache: "LmCache", slot: int, ids, score: bool = False):
        """Append ``ids`` (1-D, on the device) to ``slot``.  ``score=True`` also returns f32 ``[len]``: entry t = -log P(ids[t] | the slot's
        tokens, ids[:t]) -- what ``token_nll_given`` returns for the same ids, bit for bit; entry 0 is 0 on an empty slot."""
        return self._ctx_step(cache, self._ids(ids, "ids"), [(0, ids.numel(), slot, CTX_COMMIT | (CTX_SCORE if score else 0))])

    def token_nll_given(self, cache: "LmCache", hyps: Sequence, slots=0) -> list:
        """One f32 ``[len_n]`` tensor per hypothesis: entry t = -log P(hyp[t] | the slot's tokens, hyp[:t]).  ``slots``: one slot for all
        hypotheses (an n-best list of one context) or one per hypothesis.  The cache is unchanged, and a hypothesis's values do not depend
        on the hypotheses scored beside it, bit for bit."""
        import torch
        if not len(hyps):
            return []
        slots = [int(slots)] * len(hyps) if np.ndim(slots) == 0 else [int(v) for v in slots]
        if len(slots) != len(hyps):
            raise ValueError(f"{len(slots)} slots for {len(hyps)} hypotheses")
        ids = [self._ids(t, "every hypothesis") for t in hyps]
        lens = [t.numel() for t in ids]
        offs = np.concatenate([[0], np.cumsum(lens)])
        tokens = torch.cat(ids)
        out = []
        for a in range(0, len(ids), CTX_MAX_SEQS):
            b = min(a + CTX_MAX_SEQS, len(ids))
            nll = self._ctx_step(cache, tokens, [(int(offs[n]), lens[n], slots[n], CTX_SCORE) for n in range(a, b)])
            out += list(torch.split(nll, lens[a:b]))
        return out


CTX_SCORE, CTX_COMMIT, CTX_MAX_SEQS = 1, 2, 64


class LmCache:
    """K/V cache of ``GPT2LMHeadModelMI355X``: ``slots`` contexts that ``append`` extends and ``token_nll_given`` reads.  A slot's length is
    host-side state that changes when a call is enqueued; use a cache from one thread and one stream at a time."""

    def __init__(self, model: GPT2LMHeadModelMI355X, slots: int):
        import torch
        self.model, self.slots, self._h = model, slots, None
        with torch.cuda.device(model.device):
            self._h = model._lib.loco_lm_cache_create(model._h, slots)
        if not self._h:
            raise ValueError(model._lib.loco_last_error().decode(errors="replace"))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.model._lib.loco_lm_cache_destroy(h)

    def reset(self, slot: int):
        if self.model._lib.loco_lm_cache_reset(self._h, slot) < 0:
            raise ValueError(self.model._lib.loco_last_error().decode(errors="replace"))

    def length(self, slot: int) -> int:
        n = self.model._lib.loco_lm_cache_length(self._h, slot)
        if n < 0:
            raise ValueError(f"slot = {slot} is outside 0 .. {self.slots - 1}")
        return n


def rescore(model: GPT2LMHeadModelMI355X, context_ids, hyps: Sequence):
    """N hypotheses of one utterance against a shared context: the context is encoded ONCE into a private slot, then every hypothesis is
    scored behind it.  Returns (list of f32 ``[len_n]`` NLLs, f64 ``[N]`` totals, each summed on the device in an order that depends on
    its length only).  ``context_ids`` may be empty (1-D, numel 0): every hypothesis's first token then scores 0."""
    import torch
    model._need_cuda(context_ids, "context_ids")
    longest = max((t.numel() for t in hyps), default=0)
    if context_ids.numel() + longest > model.n_positions:
        raise ValueError(f"context ({context_ids.numel()} tokens) + the longest hypothesis ({longest}) exceed n_positions = {model.n_positions}")
    cache = getattr(model, "_rescore_cache", None)
    if cache is None:
        cache = model._rescore_cache = model.new_cache(1)
    cache.reset(0)
    if context_ids.numel():
        model.append(cache, 0, context_ids)
    nlls = model.token_nll_given(cache, hyps, slots=0)
    totals = torch.stack([t.double().sum() for t in nlls]) if nlls else torch.zeros(0, dtype=torch.float64, device=model.device)
    return nlls, totals


# ---- corpus walkers: the reference's two context modes ------------------------------------------------------------------------------
class TokenizedLines:
    """The tokenizer of a ``--tokenized`` input file: the text of a line is its ids in decimal."""

    def __init__(self, eos_token_id: int, bos_token_id: Optional[int] = None):
        self.eos_token_id = eos_token_id
        self.bos_token_id = eos_token_id if bos_token_id is None else bos_token_id

    def __call__(self, text: str) -> dict:
        return {"input_ids": [int(t) for t in text.split()]}


def read_key_text(path: str) -> "OrderedDict[str, str]":
    """``utt_id text`` lines -> {utt_id: text} in file order; a repeated utt_id keeps its first line (the reference prints and ignores)."""
    utts: "OrderedDict[str, str]" = OrderedDict()
    with open(path, "r", encoding="utf-8") as fh:
        for n, line in enumerate(fh, 1):
            parts = line.strip().split(None, 1)
            if len(parts) != 2:
                raise ValueError(f"{path}:{n}: expected 'utt_id text', got {line.strip()!r}")
            utts.setdefault(parts[0], parts[1])
    return utts


def rec_id_of(utt_id: str) -> str:
    return utt_id.split("-", 1)[0]


def indep_plan(utts: "Dict[str, str]", tokenizer, bsize: int = 128) -> Tuple[List[str], List[List[int]], List[Tuple[int, int]]]:
    """``indep`` mode: ``<bos> ids <eos>`` per utterance, sorted by length (numpy's default argsort, as the reference sorts), cut into
    batches of at most ``bsize`` utterances of EQUAL length.  Returns (utt_ids, id lists, [(first, last + 1) of every batch]) in sorted
    order; every position of an utterance but the last is scored."""
    ids, keys = [], []
    for utt_id, text in utts.items():
        ids.append([tokenizer.bos_token_id] + list(tokenizer(text)["input_ids"]) + [tokenizer.eos_token_id])
        keys.append(utt_id)
    lengths = np.asarray([len(t) for t in ids])
    order = np.argsort(lengths)
    ids, keys, lengths = [ids[i] for i in order], [keys[i] for i in order], lengths[order]
    batches, a = [], 0
    while a < len(ids):
        b = a
        while b < len(ids) and lengths[b] == lengths[a] and b - a < bsize:
            b += 1
        batches.append((a, b))
        a = b
    return keys, ids, batches


def recordings(utts: "Dict[str, str]", tokenizer, utt_lens: Optional[dict] = None) -> "OrderedDict[str, List[int]]":
    """``max_len`` mode's sequences: per recording its utterances in (rec, start, end) order -- utt_id is ``rec-x-start-end`` and the key
    is the STRING ``rec-start-end``, as the reference sorts -- each followed by ``<eos>``, no ``<bos>``.  ``utt_lens`` (a dict, optional)
    receives per recording the token count of every utterance, its ``<eos>`` included: ``carry`` mode's chunks."""

    def key(utt_id):
        parts = utt_id.split("-")
        if len(parts) != 4:
            raise ValueError(f"utt_id {utt_id!r} is not of the form rec-x-start-end, which max_len mode sorts by")
        return "-".join((parts[0], parts[2], parts[3]))

    recs: "OrderedDict[str, List[int]]" = OrderedDict()
    for utt_id in sorted(utts, key=key):
        seq = recs.setdefault(rec_id_of(utt_id), [])
        n0 = len(seq)
        seq.extend(tokenizer(utts[utt_id])["input_ids"])
        seq.append(tokenizer.eos_token_id)
        if utt_lens is not None:
            utt_lens.setdefault(rec_id_of(utt_id), []).append(len(seq) - n0)
    return recs


def max_len_plan(n_tokens: int, max_len: int, bsize: int, strict_reference: bool = True) -> Iterator[Tuple[List[int], bool, bool]]:
    """The windows of one recording of ``n_tokens`` tokens, as (window start offsets, first, last) per batch, in the reference's order:
    shorter than ``max_len``: one batch ``([0], True, True)`` holding the whole recording; otherwise windows of ``max_len`` tokens at
    offsets 0 .. n - max_len - 1 -- offset 0 alone in a first batch (scored in full), the rest in batches of ``bsize`` (each scored on
    its last position).  ``last`` marks the batch that holds the final window.  See the module docstring for the two quirks."""
    if n_tokens < max_len:
        yield [0], True, True
        return
    n_win = n_tokens - max_len + (0 if strict_reference else 1)
    if n_win <= 0:
        return
    yield [0], True, n_win == 1
    for a in range(1, n_win, bsize):
        b = min(a + bsize, n_win)
        yield list(range(a, b)), False, b == n_win


def fold_offsets(rec_ids: Sequence[str], counts: Sequence[int]):
    """Group items by recording, recordings in order of first appearance: (recording names, permutation of the flat NLL buffer that
    makes every recording contiguous, offsets [G + 1])."""
    names: "OrderedDict[str, List[Tuple[int, int]]]" = OrderedDict()
    pos = 0
    for rid, n in zip(rec_ids, counts):
        names.setdefault(rid, []).append((pos, n))
        pos += n
    perm, offsets = [], [0]
    for spans in names.values():
        for a, n in spans:
            perm.append(np.arange(a, a + n))
        offsets.append(offsets[-1] + sum(n for _, n in spans))
    return list(names), (np.concatenate(perm) if perm else np.zeros(0, np.int64)), np.asarray(offsets, np.int64)


def fold_ppl(nll, rec_ids: Sequence[str], counts: Sequence[int]):
    """Per-recording fold on the device: ``nll`` is the flat f32 buffer of every scored token, item i owning ``counts[i]`` of them and
    belonging to recording ``rec_ids[i]``.  Returns ({rec: [nll, ...]}, {rec: ppl}) with ppl = exp(mean nll), the mean taken in double
    on the device in a fixed order."""
    import torch
    names, perm, offsets = fold_offsets(rec_ids, counts)
    if int(offsets[-1]) != nll.numel():
        raise ValueError(f"{nll.numel()} NLLs but the items count {int(offsets[-1])}")
    lib = _lib.load()
    dev = nll.device
    grouped = nll.contiguous()[torch.as_tensor(perm, device=dev)].contiguous()
    d_off = torch.as_tensor(offsets.astype(np.int32), device=dev)
    mean = torch.empty(len(names), dtype=torch.float64, device=dev)
    ppl = torch.empty_like(mean)
    with torch.cuda.device(dev):
        _lib.check(lib.loco_op_lm_group_mean(C.c_void_p(grouped.data_ptr()), C.c_void_p(d_off.data_ptr()), len(names), C.c_void_p(mean.data_ptr()),
                                             C.c_void_p(ppl.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "loco_op_lm_group_mean")
    host = grouped.cpu().numpy()
    rec_id2nlls = {r: host[offsets[g]:offsets[g + 1]].astype(np.float64).tolist() for g, r in enumerate(names)}
    return rec_id2nlls, dict(zip(names, ppl.cpu().tolist()))


def score_indep(model: GPT2LMHeadModelMI355X, utts, tokenizer, bsize: int = 128):
    """``indep`` mode over a corpus: (rec_id2nlls, rec_id2ppl)."""
    import torch
    keys, ids, batches = indep_plan(utts, tokenizer, bsize)
    lens = np.asarray([len(t) for t in ids], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)])
    tokens = torch.as_tensor(np.concatenate([np.asarray(t, np.int32) for t in ids]), device=model.device or "cuda")
    out = []
    for a, b in batches:
        S = int(lens[a])
        rows = (np.arange(b - a)[:, None] * S + np.arange(S - 1)[None, :]).reshape(-1)
        out.append(model.nll_rows(tokens, offs[a:b], lens[a:b], S, rows))
    return fold_ppl(torch.cat(out), [rec_id_of(k) for k in keys], (lens - 1).tolist())


def score_max_len(model: GPT2LMHeadModelMI355X, utts, tokenizer, bsize: int = 128, max_len: Optional[int] = None, strict_reference: bool = True):
    """``max_len`` mode over a corpus: (rec_id2nlls, rec_id2ppl).  A recording's ids are uploaded once; every window is a (start,
    length) pair into that buffer.  Absolute positions restart in every window, so nothing is reused between windows."""
    import torch
    max_len = max_len or model.n_positions
    out, rec_ids, counts = [], [], []
    for rec, seq in recordings(utts, tokenizer).items():
        if len(seq) < 2:
            continue
        tokens = torch.as_tensor(np.asarray(seq, np.int32), device=model.device or "cuda")
        for starts, first, _last in max_len_plan(len(seq), max_len, bsize, strict_reference):
            S = min(len(seq), max_len)
            rows = np.arange(S - 1) if first else np.arange(len(starts)) * S + (S - 2)
            out.append(model.nll_rows(tokens, starts, [S] * len(starts), S, rows))
            rec_ids.append(rec)
            counts.append(len(rows))
    if not out:
        return {}, {}
    return fold_ppl(torch.cat(out), rec_ids, counts)


# ---- a third context mode: carry -----------------------------------------------------------------------------------------------------
def carry_plan(chunk_lens: Sequence[int], n_positions: int, keep: Optional[int] = None) -> Iterator[Tuple[int, int, int, int, bool]]:
    """``carry`` mode's walk of one recording whose utterances have ``chunk_lens`` tokens: (base, P, chunk_start, chunk_end, rebased) per
    chunk, all offsets into the recording's token stream.  A chunk is one utterance; an utterance longer than ``n_positions - keep`` is
    cut into pieces of that size.  The slot holds stream tokens [base, base + P) when the chunk [chunk_start, chunk_end) is scored behind
    them and appended.  A chunk that does not fit (P + L > n_positions) first rebases the slot: it is reset and re-prefilled with the
    last ``keep`` stream tokens before the chunk (base = chunk_start - keep, P = keep).  Pure host arithmetic."""
    keep = n_positions // 2 if keep is None else keep
    if not 1 <= keep < n_positions:
        raise ValueError(f"keep = {keep} must satisfy 1 <= keep < n_positions = {n_positions}")
    piece = n_positions - keep
    base = P = pos = 0
    for n in chunk_lens:
        if n < 1:
            raise ValueError(f"a chunk of {n} tokens")
        for a in range(0, n, piece):
            L = min(piece, n - a)
            rebased = P + L > n_positions
            if rebased:
                base, P = pos - keep, keep
            yield base, P, pos, pos + L, rebased
            P += L
            pos += L


def score_carry(model: GPT2LMHeadModelMI355X, utts, tokenizer, keep: Optional[int] = None, inflight: int = 8):
    """``carry`` mode over a corpus: (rec_id2nlls, rec_id2ppl).  Every token of a recording but its very first is scored exactly once,
    behind everything since the recording's start until the slot fills, then behind the last ``keep`` .. ``n_positions - 1`` tokens
    (``carry_plan``).  This is HuggingFace's strided perplexity with utterance-aligned strides, NOT the reference's ``max_len``, which
    gives every token the full ``n_positions - 1`` of context at the price of one forward per token.

    Up to ``inflight`` recordings are walked in lock-step, one cache slot each: per round one call re-prefills the slots that rebase
    (through the same attention kernel, P = 0) and one call scores and appends every recording's chunk.  A recording's NLLs do not depend
    on ``inflight`` or on the recordings walked beside it, bit for bit."""
    import torch
    if not 1 <= inflight <= CTX_MAX_SEQS:
        raise ValueError(f"inflight = {inflight} is outside 1 .. {CTX_MAX_SEQS}")
    utt_lens: dict = {}
    recs = [(r, seq) for r, seq in recordings(utts, tokenizer, utt_lens).items() if len(seq) >= 2]
    if not recs:
        return {}, {}
    plans = [list(carry_plan(utt_lens[r], model.n_positions, keep)) for r, _ in recs]
    offs = np.concatenate([[0], np.cumsum([len(seq) for _, seq in recs])])
    dev = model.device or "cuda"
    tokens = torch.as_tensor(np.concatenate([np.asarray(seq, np.int32) for _, seq in recs]), device=dev)
    cache = model.new_cache(min(inflight, len(recs)), dev)
    out, rec_ids, counts = [], [], []
    for g0 in range(0, len(recs), inflight):
        group = range(g0, min(g0 + inflight, len(recs)))
        for i in group:
            cache.reset(i - g0)
        for rnd in range(max(len(plans[i]) for i in group)):
            live = [i for i in group if rnd < len(plans[i])]
            rebase = [i for i in live if plans[i][rnd][4]]
            for i in rebase:
                cache.reset(i - g0)
            if rebase:  # phase A: the last `keep` tokens before the chunk, committed and not scored
                model._ctx_step(cache, tokens, [(int(offs[i]) + plans[i][rnd][0], plans[i][rnd][1], i - g0, CTX_COMMIT) for i in rebase])
            # phase B: every live recording's chunk, scored behind its slot and appended to it
            nll = model._ctx_step(cache, tokens, [(int(offs[i]) + plans[i][rnd][2], plans[i][rnd][3] - plans[i][rnd][2], i - g0, CTX_SCORE | CTX_COMMIT)
                                                  for i in live])
            for i, piece in zip(live, torch.split(nll, [plans[i][rnd][3] - plans[i][rnd][2] for i in live])):
                piece = piece[1:] if rnd == 0 else piece  # the recording's very first token: nothing predicts it
                if piece.numel():
                    out.append(piece)
                    rec_ids.append(recs[i][0])
                    counts.append(piece.numel())
    return fold_ppl(torch.cat(out), rec_ids, counts)
