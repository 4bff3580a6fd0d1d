"""Drop-in for the reference's TEXT branch: ``SpeechT5ForTextToSpeech(...).speecht5.encoder``.

/root/reference/speech_text/extract_speecht5_base_embeddings_slurp.py:79-93 loads a ``wrapped_encoder`` and a text
``prenet`` state dict into HF's ``SpeechT5EncoderWithTextPrenet`` and calls ``model.speecht5.encoder(texts.input_ids)``
-- token ids only, no attention mask -- keeping ``out.last_hidden_state``.  HF (modeling_speecht5.py,
``SpeechT5TextEncoderPrenet`` / ``SpeechT5ScaledPositionalEncoding`` / ``SpeechT5EncoderWithTextPrenet``):
``hidden = embed_tokens(ids) + alpha * pe[:, :T]`` followed by the same 12-layer encoder the speech path uses.

The arithmetic runs in ``libloco_asr.so`` (``loco_forward_text``); this module only keeps HF's names and call contract.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import nn

from . import _lib
from .encoder import HIDDEN, LAYERS, Pack, _EncoderBase
from .holders import _Ref, _WeightHolder
from .speech_to_text import _SpeechT5Core

VOCAB_SIZE = 81           # SpeechT5Config.vocab_size
MAX_TEXT_POSITIONS = 450  # SpeechT5Config.max_text_positions
PAD_TOKEN_ID = 1


def scaled_positional_table(rows: int, dim: int = HIDDEN) -> torch.Tensor:
    """SpeechT5ScaledPositionalEncoding.__init__ -- the same torch expression, so the table is bit-identical to HF's."""
    pe = torch.zeros(rows, dim)
    position = torch.arange(0, rows).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, dim, 2, dtype=torch.int64).float() * -(math.log(10000.0) / dim))
    pe[:, 0::2] = torch.sin(position.float() * div_term)
    pe[:, 1::2] = torch.cos(position.float() * div_term)
    return pe


class SpeechT5TextEncoderPrenetMI355X(_WeightHolder):
    """Parameter names of HF SpeechT5TextEncoderPrenet: ``embed_tokens.weight`` [vocab,768], ``encode_positions.alpha`` []."""

    def __init__(self, owner_ref, vocab_size: int = VOCAB_SIZE):
        super().__init__(owner_ref)
        emb = nn.Module()
        emb.register_parameter("weight", nn.Parameter(torch.zeros(vocab_size, HIDDEN), requires_grad=False))
        self.add_module("embed_tokens", emb)
        pos = nn.Module()
        pos.register_parameter("alpha", nn.Parameter(torch.tensor(1.0), requires_grad=False))
        self.add_module("encode_positions", pos)

    def _translate(self, sd):
        # transformers 4.30.2 (the reference's pin) registers the table as a persistent buffer and the reference's pickled
        # dict carries it (map_speecht5_hf.py:168-181); it is a constant of (max_len, dim) and is rebuilt here
        sd.pop("encode_positions.pe", None)
        return sd


class SpeechT5EncoderWithTextPrenetMI355X(_EncoderBase):
    """``forward(input_values=ids [B,T], attention_mask=None, ...) -> BaseModelOutput`` like HF's class of the same name: the text
    front end of encoder.py's ``_EncoderBase``, which owns ``forward``, ``forward_async`` and everything they share with speech."""

    def __init__(self, layers: int = LAYERS, precision: str = "f16x3", vocab_size: int = VOCAB_SIZE,
                 max_text_positions: int = MAX_TEXT_POSITIONS):
        super().__init__(SpeechT5TextEncoderPrenetMI355X(_Ref(), vocab_size), layers, precision, streams=1)
        self.vocab_size = vocab_size
        self.max_text_positions = max_text_positions

    def _weight_sources(self):
        return [("text_prenet.", self.prenet), ("wrapped_encoder.", self.wrapped_encoder)]

    def _load_tables(self, put, dirty, min_rows):
        if dirty:
            put("text_prenet.encode_positions.pe", scaled_positional_table(self.max_text_positions))

    def _prepare(self, input_values, attention_mask):
        ids32, m = self._check_ids(input_values, attention_mask)
        return ids32, m, ids32.shape[1]

    def _workspace_need(self, B, T):
        return int(self._lib.loco_text_workspace_bytes(self._handle, B, T))

    def _check_ids(self, ids, attention_mask):
        if ids.dim() != 2 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise ValueError(f"input_values must be integer token ids [batch, tokens], got {ids.dtype} {tuple(ids.shape)}")
        B, T = ids.shape
        if T < 1 or B < 1:
            raise ValueError("empty batch")
        if T > self.max_text_positions:
            raise ValueError(f"{T} tokens exceed max_text_positions = {self.max_text_positions}")
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= self.vocab_size:
            raise IndexError(f"token id out of range [0, {self.vocab_size}): min {lo}, max {hi}")  # nn.Embedding raises IndexError too
        m = None
        if attention_mask is not None:
            if attention_mask.shape != ids.shape:
                raise ValueError(f"attention_mask {tuple(attention_mask.shape)} does not match input_values {tuple(ids.shape)}")
            m = attention_mask.to(device=ids.device, dtype=torch.int32).contiguous()
            if T > 1 and not bool((m[:, 1:] <= m[:, :-1]).all()):
                raise NotImplementedError("attention_mask must be right padding (ones then zeros), as the tokenizer produces it")
        return ids.to(torch.int32).contiguous(), m

    def _launch(self, slot, ids32, m, out, frames, precision, pack, hidden):  # pack / hidden: unused (a text pack is an ordinary masked forward)
        B, T = ids32.shape
        _lib.check(self._lib.loco_forward_text_async(
            self._handle, self.PRECISIONS[precision], C.c_void_p(ids32.data_ptr()), C.c_void_p(m.data_ptr()) if m is not None else None, B, T,
            C.c_void_p(out.data_ptr()), C.c_void_p(frames.data_ptr()), None, C.c_void_p(slot.workspace.data_ptr()), slot.workspace.numel(),
            C.c_void_p(slot.stream.cuda_stream), C.c_void_p(slot.status.data_ptr())), "loco_forward_text_async")

    def _forward_call(self, args, stream):
        """loco_forward_text under the module's range policy (include/loco_asr.h, 'numeric range of precision mode f16x3'): the
        library has no checked text call, so the status is read here and the batch run again on the exact-fp32 kernels (the
        re-run rewrites the bound attention buffers too)."""
        _lib.check(self._lib.loco_forward_text(self._handle, *args, stream), "loco_forward_text")
        if self.range_policy == "off" or self.precision == "f32":
            return
        torch.cuda.current_stream(self._handle_device).synchronize()
        rc = self._lib.loco_forward_status(self._handle, None, 0)
        if rc != 0:
            if self.range_policy == "raise":
                _lib.check(rc, "loco_forward_text")
            _lib.check(self._lib.loco_set_precision(self._handle, self.PRECISIONS["f32"]), "set_precision")
            _lib.check(self._lib.loco_forward_text(self._handle, *args, stream), "loco_forward_text")
            self.last_range_fallback = True

    # -- several batches of transcripts in one forward (the reference's text loop is batch_size = 2 as well, …base…py:67-68,79-93) ----
    @torch.no_grad()
    def forward_packed_async(self, batches=None, *, packed=None):
        """Several of the reference's text batches (…base…py:79-93: ids padded to the batch's longest transcript with <pad> = 1,
        NO attention mask -- the pads of a batch attend like tokens) as ONE forward: rows of all batches side by side, padded to the
        pack's longest, and a key mask that ends every row where ITS OWN batch ends -- which is all a text batch's composition
        means here (no GroupNorm, no positional conv: the text prenet is row-wise, positions count from 0 in every row).  A batch
        given as a mapping with ``attention_mask`` (right padding) keeps that mask.  ``ticket.result()`` = one BaseModelOutput per
        batch, ``last_hidden_state`` [B_i, T_i, 768] equal to the batch's own forward up to the fp32 summation order of the GEMMs."""
        if not batches:
            raise ValueError("forward_packed: no batches")
        device = self._device()
        self._begin_async(device)
        ids_l = [b["input_values"] if hasattr(b, "keys") else b for b in batches]
        msk_l = [b.get("attention_mask") if hasattr(b, "keys") else None for b in batches]
        B, T = sum(int(i.shape[0]) for i in ids_l), max(int(i.shape[1]) for i in ids_l)
        ids = torch.full((B, T), 1, dtype=torch.int64)
        mask = torch.zeros((B, T), dtype=torch.int32)
        spans, b0 = [], 0
        for i, mk in zip(ids_l, msk_l):
            nb, t = int(i.shape[0]), int(i.shape[1])
            ids[b0:b0 + nb, :t] = i.to("cpu")
            mask[b0:b0 + nb, :t] = 1 if mk is None else mk.to("cpu", torch.int32)
            spans.append((b0, nb, t))
            b0 += nb
        ids32, m, T = self._prepare(ids.to(device), mask.to(device))
        return self._submit(ids32, m, T, Pack(wav=ids32, mask=m, valid_len=None, pad_len=[], spans=spans))


class SpeechT5ForTextToSpeechMI355X(nn.Module):
    """Only as much of HF's SpeechT5ForTextToSpeech as the reference touches: ``.speecht5.encoder`` (…base…py:80-86)."""

    def __init__(self, layers: int = LAYERS, precision: str = "f16x3"):
        super().__init__()
        self.speecht5 = _SpeechT5Core(SpeechT5EncoderWithTextPrenetMI355X(layers, precision))
        self.eval()

    @classmethod
    def from_state_dicts(cls, text_prenet_state_dict, encoder_state_dict, layers: int = LAYERS, precision: str = "f16x3"):
        model = cls(layers, precision)
        model.speecht5.encoder.wrapped_encoder.load_state_dict(encoder_state_dict)
        model.speecht5.encoder.prenet.load_state_dict(text_prenet_state_dict)
        return model
