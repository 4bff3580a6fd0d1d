"""The decoder half of ``SpeechT5ForSpeechToTextMI355X``: weight holders with HuggingFace's parameter names and the host side of
the C ABI's ``loco_decoder_*`` entry points (include/loco_asr.h).

    predicted_ids = model_stt.generate(**audios, max_length=100)
    out_stt       = model_stt(**audios, decoder_input_ids=predicted_ids)

``SpeechT5DecoderWithTextPrenetMI355X`` (``.prenet``, ``.wrapped_decoder``) and ``SpeechT5TextDecoderPostnetMI355X`` only own
parameters, so that ``load_state_dict`` of HF's dicts works; every FLOP runs in the HIP kernels of csrc/decoder.hip (the decode step)
and the library's exact-fp32 GEMM / LayerNorm (the teacher-forced pass); csrc/decoder_probs.hip forms the attention probabilities of
``output_attentions=True`` and the token timestamps of ``align``.  ``generate`` / ``generate_many`` are greedy search only: beam search,
sampling keywords, prefixes and a decoder attention mask raise by name.  Sampling has entry points of its own, ``sample`` / ``sample_many``
(temperature, top-k, top-p; csrc/decoder_sample.hip draws in the slot pool).  Scores -- the ``labels=`` loss, per-token and per-transcript log-probabilities -- come from
``loco_decoder_score`` (csrc/decoder_score.hip) on the logits of either path.
"""
from __future__ import annotations

import ctypes as C
import operator
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from .holders import _register, _WeightHolder
from .synth import DECODER_LAYERS, FFN, HIDDEN, MAX_TEXT_POSITIONS, TEXT_VOCAB

DECODER_START_TOKEN_ID = 2
EOS_TOKEN_ID = 2
PAD_TOKEN_ID = 1
IGNORE_INDEX = -100  # labels with this value do not count (torch's CrossEntropyLoss default, what HF pads labels with)
DEFAULT_MAX_LENGTH = 21  # what HF 5.x generate resolves for a default SpeechT5Config: max_new_tokens = 20 after the start token (pinned by g13 a_default_ids)

_UNSUPPORTED_GENERATE = ("num_beams", "do_sample", "decoder_input_ids", "decoder_attention_mask", "temperature", "top_k", "top_p",
                         "num_return_sequences", "repetition_penalty", "length_penalty", "no_repeat_ngram_size", "min_length",
                         "min_new_tokens", "forced_eos_token_id", "logits_processor", "stopping_criteria", "prefix_allowed_tokens_fn",
                         "past_key_values", "generation_config", "assistant_model", "streamer")


@dataclass
class Seq2SeqLMOutput:
    """Field-compatible stand-in for the part of transformers' Seq2SeqLMOutput this model fills."""
    logits: torch.Tensor = None
    encoder_last_hidden_state: torch.Tensor = None
    decoder_hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    loss: Optional[torch.Tensor] = None            # labels=: 0-d, the mean cross-entropy over the labels that are not -100
    token_logprobs: Optional[torch.Tensor] = None  # labels=: [B, S] log P(labels[b, t]), 0 where the label is -100
    # output_attentions=True: one fp32 tensor per layer, HF's shapes -- [B, 12, S, S], [B, 12, S, T_enc], [B, 12, T_enc, T_enc]
    decoder_attentions: Optional[Tuple[torch.Tensor, ...]] = None
    cross_attentions: Optional[Tuple[torch.Tensor, ...]] = None
    encoder_attentions: Optional[Tuple[torch.Tensor, ...]] = None


@dataclass
class TranscriptScores:
    """What ``score`` returns: ``token_logprobs`` [B, S] (0 at ignored labels), ``sequence_logprob`` [B] their sum per row, ``tokens``
    i32 [B] the labels that counted, ``loss`` 0-d = -sum / count over the batch."""
    token_logprobs: torch.Tensor = None
    sequence_logprob: torch.Tensor = None
    tokens: torch.Tensor = None
    loss: torch.Tensor = None


FRAME_SECONDS = 320 / 16000  # the conv stack's stride: one encoder frame every 20 ms


@dataclass
class TokenAlignment:
    """What ``align`` returns: token s of row b was spoken in the encoder frames ``start_frames[b, s]`` .. ``end_frames[b, s]`` (exclusive),
    i32 [B, S], -1 where the label is -100.  ``start_times`` / ``end_times`` f32 [B, S] are those frames x 320 / 16000 seconds (-1 where
    the frame is -1); the conv stack's receptive-field offset (a frame sees 400 samples, not 320) is ignored.  ``attention`` (on request)
    is the matrix the path was found on: f32 [B, S, T_enc], the mean cross-attention of the selected (layer, head) pairs."""
    start_frames: torch.Tensor = None
    end_frames: torch.Tensor = None
    start_times: torch.Tensor = None
    end_times: torch.Tensor = None
    attention: Optional[torch.Tensor] = None


def _ptr(t):
    """``t``'s address for the C ABI, None (a null pointer) for None."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def alignment_counts(labels_host: torch.Tensor) -> torch.Tensor:
    """n_b of every row of checked labels: the labels that count.  For an alignment -100 may only be a suffix of a row (a token
    between two ignored ones has no place on a monotone path): ValueError naming the first counted label after an ignored one."""
    counted = labels_host != IGNORE_INDEX
    n = counted.sum(dim=1)
    late = counted & (torch.arange(labels_host.shape[1])[None, :] >= n[:, None])
    if bool(late.any()):
        b, t = (int(v) for v in late.nonzero()[0])
        first = int((~counted[b]).nonzero()[0])
        raise ValueError(f"align: labels[{b}, {first}] = {IGNORE_INDEX} is followed by the counted label labels[{b}, {t}] = {int(labels_host[b, t])}; "
                         f"{IGNORE_INDEX} may only pad the end of a row")
    return n.to(torch.int32)


def check_alignment_heads(alignment_heads, layers: int, heads: int = 12):
    """None (every pair) or distinct (layer, head) pairs as a flat ctypes i32 array and their number; ValueError naming the offender."""
    if alignment_heads is None:
        return None, 0
    pairs = [tuple(int(v) for v in p) for p in alignment_heads]
    if not pairs or any(len(p) != 2 for p in pairs):
        raise ValueError("alignment_heads must be a non-empty list of (layer, head) pairs")
    for l, h in pairs:
        if not (0 <= l < layers and 0 <= h < heads):
            raise ValueError(f"alignment_heads: (layer {l}, head {h}) is outside {layers} layers x {heads} heads")
    if len(set(pairs)) != len(pairs):
        raise ValueError("alignment_heads names a (layer, head) pair twice")
    return (C.c_int32 * (2 * len(pairs)))(*[v for p in pairs for v in p]), len(pairs)


@dataclass
class GreedySearchOutput:
    """``generate(return_dict_in_generate=True)``: ``sequences`` is what ``generate`` returns otherwise.  With ``output_scores=True``
    also ``scores`` (S - 1 tensors [B, vocab]: the raw logits each step chose from), ``token_logprobs`` [B, S - 1] (entry t =
    log P(sequences[:, t + 1]); 0 at the <pad> columns of a row that had ended) and ``sequence_logprobs`` [B]."""
    sequences: torch.Tensor = None
    scores: Optional[Tuple[torch.Tensor, ...]] = None
    token_logprobs: Optional[torch.Tensor] = None
    sequence_logprobs: Optional[torch.Tensor] = None


@dataclass
class SampleOutput:
    """What ``sample`` returns: ``sequences`` [B * N, S] in HF's num_return_sequences layout (clip b's hypotheses in rows b * N ..
    b * N + N - 1, <pad> after </s>), ``seed`` the Philox seed that was used; with ``return_scores=True`` also ``token_logprobs``
    [B * N, S - 1] (entry t = the model's log P(sequences[:, t + 1]), 0 at the <pad> columns) and ``sequence_logprobs`` [B * N]."""
    sequences: torch.Tensor = None
    token_logprobs: Optional[torch.Tensor] = None
    sequence_logprobs: Optional[torch.Tensor] = None
    seed: int = None


class SampledHypotheses(list):
    """``sample_many``'s hypotheses, ``hyps[u][h]``; ``seed`` is the Philox seed that was used."""
    seed = None


class SampledResults(tuple):
    """``sample_many``'s (hypotheses, logits and / or scores); ``seed`` as on the hypotheses."""
    seed = None


MAX_RETURN_SEQUENCES = 64


def check_sample_args(num_return_sequences, temperature, top_k, top_p, seed):
    """(N, a _lib.SampleConfig) of checked sampling arguments; ValueError naming the offender.  ``seed=None`` draws 63 bits from
    torch's default CPU generator (``torch.manual_seed`` makes the call reproducible)."""
    try:
        n = operator.index(num_return_sequences)
    except TypeError:
        raise ValueError(f"num_return_sequences must be an integer in 1 .. {MAX_RETURN_SEQUENCES}, got {num_return_sequences!r}") from None
    if not 1 <= n <= MAX_RETURN_SEQUENCES:
        raise ValueError(f"num_return_sequences = {n} is outside 1 .. {MAX_RETURN_SEQUENCES}")
    t = float(temperature)
    if not (t > 0 and t != float("inf")):
        raise ValueError(f"temperature = {temperature} must be finite and > 0")
    try:
        k = operator.index(top_k)
    except TypeError:
        raise ValueError(f"top_k must be an integer >= 0 (0 = off), got {top_k!r}") from None
    if not 0 <= k < 2 ** 31:
        raise ValueError(f"top_k = {k} must be >= 0 (0 = off)")
    p = float(top_p)
    if not 0 < p <= 1:
        raise ValueError(f"top_p = {top_p} is outside (0, 1] (1 = off)")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
    seed = operator.index(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed = {seed} is outside 0 .. 2^64 - 1")
    return n, _lib.SampleConfig(C.sizeof(_lib.SampleConfig), t, k, p, seed)


MAX_BEAMS = 16
EARLY_STOPPING = {False: 0, True: 1, "never": 2}


@dataclass
class BeamSearchOutput:
    """What ``beam_search`` returns, in HF's ``num_return_sequences`` layout: ``sequences`` [B * N, S] (clip b's hypotheses, best
    first, in rows b * N .. b * N + N - 1, <pad> after the end), ``sequences_scores`` f64 [B * N] (HF's: the sum of the tokens'
    log-probabilities over length ** length_penalty), ``token_logprobs`` [B * N, S - 1] (0 at the <pad> columns) and
    ``sequence_logprobs`` f64 [B * N]."""
    sequences: torch.Tensor = None
    sequences_scores: Optional[torch.Tensor] = None
    token_logprobs: Optional[torch.Tensor] = None
    sequence_logprobs: Optional[torch.Tensor] = None
    lm_logprobs: Optional[torch.Tensor] = None  # with lm=: float64 [B * N], the hypotheses' n-gram log-probabilities


class BeamHypotheses(list):
    """``beam_search_many``'s hypotheses, ``hyps[u][h]`` best first; ``sequence_scores[u]`` f64 [N] are HF's ``sequences_scores`` and
    ``sequence_logprobs[u]`` f64 [N] the sums of the tokens' log-probabilities.  With ``lm=`` both are the FUSED values (every token's
    log P plus ``lm_weight`` * its n-gram log P plus ``lm_bonus``) and ``lm_logprobs[u]`` f64 [N] are the hypotheses' n-gram
    log-probabilities; without, ``lm_logprobs`` is None."""
    sequence_scores = None
    sequence_logprobs = None
    lm_logprobs = None


def check_fusion_args(lm, lm_weight=0.0, lm_bonus=0.0, vocab=None):
    """None, or (lm, weight, bonus) of checked shallow-fusion arguments; ValueError naming the offender."""
    if lm is None:
        if float(lm_weight) != 0.0 or float(lm_bonus) != 0.0:
            raise ValueError("lm_weight / lm_bonus need lm=, an ngram.NgramLM")
        return None
    if not (hasattr(lm, "vocab") and hasattr(lm, "next_logprobs")):
        raise ValueError(f"lm must be an ngram.NgramLM, got {type(lm).__name__}")
    if vocab is not None and int(lm.vocab) != int(vocab):
        raise ValueError(f"lm: the model's vocab = {int(lm.vocab)} is not the decoder's {int(vocab)}")
    out = []
    for name, v in (("lm_weight", lm_weight), ("lm_bonus", lm_bonus)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a finite number, got {v!r}") from None
        if f != f or f in (float("inf"), float("-inf")):
            raise ValueError(f"{name} = {v} must be finite")
        out.append(f)
    return lm, out[0], out[1]


def check_beam_args(num_beams, num_return_sequences=None, length_penalty=1.0, early_stopping=False, vocab=None):
    """(K, N, a _lib.BeamConfig) of checked beam-search arguments; ValueError naming the offender.  ``num_return_sequences=None`` is
    1, as in HF; ``early_stopping`` is False, True or "never"; ``vocab`` (when known) must hold 2 * num_beams candidates."""
    try:
        k = operator.index(num_beams)
    except TypeError:
        raise ValueError(f"num_beams must be an integer in 1 .. {MAX_BEAMS}, got {num_beams!r}") from None
    if not 1 <= k <= MAX_BEAMS:
        raise ValueError(f"num_beams = {k} is outside 1 .. {MAX_BEAMS}")
    if vocab is not None and 2 * k > int(vocab):
        raise ValueError(f"num_beams = {k} needs 2 * num_beams <= the vocabulary's {int(vocab)} tokens")
    try:
        n = 1 if num_return_sequences is None else operator.index(num_return_sequences)
    except TypeError:
        raise ValueError(f"num_return_sequences must be an integer in 1 .. num_beams, got {num_return_sequences!r}") from None
    if not 1 <= n <= k:
        raise ValueError(f"num_return_sequences = {n} is outside 1 .. num_beams = {k}")
    try:
        p = float(length_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"length_penalty must be a finite number, got {length_penalty!r}") from None
    if p != p or p in (float("inf"), float("-inf")):
        raise ValueError(f"length_penalty = {length_penalty} must be finite")
    if isinstance(early_stopping, str):
        early_stopping = early_stopping.lower()
    if not isinstance(early_stopping, (bool, str)) or early_stopping not in EARLY_STOPPING:
        raise ValueError(f"early_stopping = {early_stopping!r} is not False, True or 'never'")
    return k, n, _lib.BeamConfig(C.sizeof(_lib.BeamConfig), k, p, EARLY_STOPPING[early_stopping], 0)


def decoder_layer_keys(layer: int):
    """(name below ``wrapped_decoder.``, shape, init) of one SpeechT5DecoderLayer (HF modeling_speecht5.py:1070-1100)."""
    b = f"layers.{layer}."
    for attn in ("self_attn", "encoder_attn"):
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            yield f"{b}{attn}.{proj}.weight", (HIDDEN, HIDDEN), 0.0
            yield f"{b}{attn}.{proj}.bias", (HIDDEN,), 0.0
    for ln in ("self_attn_layer_norm", "encoder_attn_layer_norm", "final_layer_norm"):
        yield f"{b}{ln}.weight", (HIDDEN,), 1.0
        yield f"{b}{ln}.bias", (HIDDEN,), 0.0
    yield f"{b}feed_forward.intermediate_dense.weight", (FFN, HIDDEN), 0.0
    yield f"{b}feed_forward.intermediate_dense.bias", (FFN,), 0.0
    yield f"{b}feed_forward.output_dense.weight", (HIDDEN, FFN), 0.0
    yield f"{b}feed_forward.output_dense.bias", (HIDDEN,), 0.0


class SpeechT5DecoderWithTextPrenetMI355X(_WeightHolder):
    """Parameter names of HF SpeechT5DecoderWithTextPrenet: ``prenet.embed_tokens.weight`` and ``wrapped_decoder.layers.N.*``
    (``prenet.embed_positions.weights`` is a non-persistent buffer in HF: not a key; the table is regenerated).  Parameter changes
    mark ``owner_ref()``'s weights dirty (the encoder module owns the library handle)."""

    def __init__(self, owner_ref, layers: int = DECODER_LAYERS, vocab: int = TEXT_VOCAB):
        super().__init__(owner_ref)
        _register(self, "prenet.embed_tokens.weight", (vocab, HIDDEN))
        self.num_layers = layers
        for l in range(layers):
            for name, shape, init in decoder_layer_keys(l):
                _register(self, "wrapped_decoder." + name, shape, init)

    def _translate(self, sd):
        sd.pop("prenet.embed_positions.weights", None)
        return sd


class SpeechT5TextDecoderPostnetMI355X(_WeightHolder):
    """Parameter name of HF SpeechT5TextDecoderPostnet: ``lm_head.weight`` (no bias)."""

    def __init__(self, owner_ref, vocab: int = TEXT_VOCAB):
        super().__init__(owner_ref)
        _register(self, "lm_head.weight", (vocab, HIDDEN))


def position_ids(input_ids: torch.Tensor, past_key_values_length: int = 0) -> torch.Tensor:
    """HF's create_position_ids_from_input_ids with padding_idx 1 (modeling_speecht5.py:337-351) -- the rule dec_embed_kernel
    implements: a token's position is the count of non-pad tokens up to and including it, plus 1; <pad> maps to row 1 (zeros)."""
    mask = input_ids.ne(PAD_TOKEN_ID).int()
    return ((torch.cumsum(mask, dim=1).type_as(mask) + past_key_values_length) * mask).long() + PAD_TOKEN_ID


def shift_tokens_right(labels: torch.Tensor, pad_token_id: int = PAD_TOKEN_ID, decoder_start_token_id: int = DECODER_START_TOKEN_ID) -> torch.Tensor:
    """HF's shift_tokens_right (modeling_speecht5.py): the decoder's input for ``labels`` -- the start token in column 0, the labels
    one column to the right, -100 replaced by <pad>."""
    shifted = labels.new_zeros(labels.shape)
    shifted[:, 1:] = labels[:, :-1]
    shifted[:, 0] = decoder_start_token_id
    return shifted.masked_fill(shifted == IGNORE_INDEX, pad_token_id)


def check_labels(labels, batch: int, vocab: int, ids_shape=None) -> torch.Tensor:
    """``labels`` as a host LongTensor [batch, S] with every value in [0, vocab) or -100; ValueError naming the offender otherwise."""
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[0] != batch or labels.shape[1] < 1:
        got = tuple(labels.shape) if torch.is_tensor(labels) else type(labels).__name__
        raise ValueError(f"labels must be a [batch, tokens] tensor with batch {batch}, got {got}")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"labels must hold integer token ids, got dtype {labels.dtype}")
    if ids_shape is not None and tuple(labels.shape) != tuple(ids_shape):
        raise ValueError(f"labels {tuple(labels.shape)} and decoder_input_ids {tuple(ids_shape)} must have the same shape")
    if labels.shape[1] > MAX_TEXT_POSITIONS:
        raise ValueError(f"labels of {labels.shape[1]} tokens exceed max_text_positions = {MAX_TEXT_POSITIONS}")
    host = labels.detach().to(device="cpu", dtype=torch.long)
    bad = ((host < 0) | (host >= vocab)) & (host != IGNORE_INDEX)
    if bool(bad.any()):
        b, t = (int(v) for v in bad.nonzero()[0])
        raise ValueError(f"labels[{b}, {t}] = {int(host[b, t])} is neither a token id in [0, {vocab}) nor {IGNORE_INDEX}")
    return host


def score_logits(lib, logits: torch.Tensor, targets: Optional[torch.Tensor], B: int, S: int, reduce: bool = True, chosen: bool = False):
    """loco_decoder_score on ``logits`` (f32, device, B * S rows of one row stride, the last dimension the vocabulary) against
    ``targets`` i32 [B, S] on the device (None: each row's argmax).  Returns (token_logprobs [B, S], sequence sums [B], counts i32 [B],
    loss 0-d, chosen i32 [B, S]); what was not asked for is None.  Enqueued on the current stream; nothing is read back."""
    if logits.dtype != torch.float32 or not logits.is_cuda:
        raise ValueError("score_logits: logits must be an fp32 device tensor (there is no CPU path)")
    V = int(logits.shape[-1])
    rows = logits.reshape(-1, V) if logits.is_contiguous() else logits
    if rows.dim() != 2 or rows.shape[0] != B * S or rows.stride(1) != 1:
        raise ValueError(f"score_logits: logits {tuple(logits.shape)} are not {B * S} rows of one stride")
    if targets is not None and (targets.dtype != torch.int32 or targets.device != logits.device or targets.numel() != B * S or not targets.is_contiguous()):
        raise ValueError("score_logits: targets must be a contiguous i32 device tensor with one entry per row")
    device = logits.device
    lp = torch.empty((B, S), dtype=torch.float32, device=device)
    seq = torch.empty((B,), dtype=torch.float32, device=device) if reduce else None
    cnt = torch.empty((B,), dtype=torch.int32, device=device) if reduce else None
    loss = torch.empty((1,), dtype=torch.float32, device=device) if reduce else None
    ch = torch.empty((B, S), dtype=torch.int32, device=device) if chosen else None
    with torch.cuda.device(device):
        _lib.check(lib.loco_decoder_score(_ptr(rows), rows.stride(0) if rows.shape[0] > 1 else V, _ptr(targets), B, S, V, IGNORE_INDEX, _ptr(lp), _ptr(ch),
                                          _ptr(seq), _ptr(cnt), _ptr(loss), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "loco_decoder_score")
    return lp, seq, cnt, (loss.reshape(()) if loss is not None else None), ch


def resolve_max_length(max_length=None, max_new_tokens=None) -> int:
    """Total length (start token included) as HF's generate resolves it: ``max_new_tokens`` counts tokens after the start token and
    wins over ``max_length``; neither given = HF's default for a default SpeechT5Config."""
    if max_new_tokens is not None:
        if int(max_new_tokens) < 1:
            raise ValueError("max_new_tokens must be >= 1")
        n = int(max_new_tokens) + 1
    elif max_length is not None:
        n = int(max_length)
    else:
        n = DEFAULT_MAX_LENGTH
    if n < 2:
        raise ValueError(f"max_length must be >= 2 (the start token and one generated token), got {n}")
    if n > MAX_TEXT_POSITIONS:
        raise ValueError(f"max_length {n} exceeds max_text_positions = {MAX_TEXT_POSITIONS}")
    return n


def check_generate_kwargs(kwargs: dict):
    """Refuse what greedy search does not cover, by name; ``num_beams=1`` / ``do_sample=False`` are what it is and pass."""
    for k, v in kwargs.items():
        if k == "num_beams" and v in (None, 1):
            continue
        if k == "do_sample" and not v:
            continue
        if k in _UNSUPPORTED_GENERATE:
            raise NotImplementedError(f"generate({k}=...) is not implemented: this decoder does greedy search from the start token only")
        raise TypeError(f"generate() got an unexpected keyword argument '{k}'")


class DecoderRuntime:
    """Host side of loco_decoder_*: workspace ownership and argument marshalling for one encoder module's handle.

    Single caller, one stream: the model keeps ONE workspace (grown on demand) and the library one pinned poll word per handle, so
    calls of one model must be issued from one thread on one stream -- a call that grows the workspace frees the old one behind the
    work already enqueued on that stream (the caching allocator's ordering), which holds for the current stream only."""

    def __init__(self, encoder):
        self.enc = encoder
        self.lib = encoder._lib
        self._workspace = None
        self.last_lengths = None  # after generate: i32 [B] on the host, every row's length

    def max_batch(self) -> int:
        return int(self.lib.loco_decoder_max_batch())

    def _grown(self, need, device):
        """The workspace, replaced by one of ``need`` bytes when it is smaller or on another device."""
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
            self._workspace = None
            self._workspace = torch.empty(need, dtype=torch.uint8, device=device)
        return self._workspace

    def workspace(self, B, T, S, device):
        return self._grown(int(self.lib.loco_decoder_workspace_bytes(self.enc._handle, B, T, S)), device)

    @staticmethod
    def _stream(device):
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def _teacher_forced(self, entry, enc_out, frames, ids, output_hidden_states, probs):
        """The teacher-forced pass through the entry point ``entry`` (loco_decoder_forward or loco_decoder_forward_attn): allocates the
        logits, the hidden states when asked for and, with ``probs``, the per-layer self- and cross-attention probabilities that
        loco_decoder_forward_attn also takes."""
        B, T, _ = enc_out.shape
        S = ids.shape[1]
        if S > MAX_TEXT_POSITIONS:
            raise ValueError(f"decoder_input_ids of {S} tokens exceed max_text_positions = {MAX_TEXT_POSITIONS}")
        device = enc_out.device
        ws = self.workspace(B, T, S, device)
        layers = self.enc._decoder_layers
        logits = torch.empty((B, S, self.enc._decoder_vocab), dtype=torch.float32, device=device)
        hs, hs_ptrs = None, None
        if output_hidden_states:
            hs = [torch.empty((B, S, HIDDEN), dtype=torch.float32, device=device) for _ in range(layers + 1)]
            hs_ptrs = (C.c_void_p * len(hs))(*[t.data_ptr() for t in hs])
        attn = ()
        if probs:
            attn = (tuple(torch.empty((B, 12, S, S), dtype=torch.float32, device=device) for _ in range(layers)),
                    tuple(torch.empty((B, 12, S, T), dtype=torch.float32, device=device) for _ in range(layers)))
        _lib.check(getattr(self.lib, entry)(self.enc._handle, _ptr(enc_out), _ptr(frames), B, T, _ptr(ids), S, _ptr(logits), hs_ptrs,
                         *[(C.c_void_p * layers)(*[t.data_ptr() for t in ts]) for ts in attn], _ptr(ws), ws.numel(), self._stream(device)),
                   entry)
        return (logits, (tuple(hs) if hs is not None else None)) + attn

    def forward(self, enc_out, frames, ids, output_hidden_states=False):
        return self._teacher_forced("loco_decoder_forward", enc_out, frames, ids, output_hidden_states, False)

    def forward_attn(self, enc_out, frames, ids, output_hidden_states=False):
        """``forward`` through loco_decoder_forward_attn: (logits, hidden states or None, self-attention P, cross-attention P), the
        last two tuples of one fp32 tensor per layer, [B, 12, S, S] and [B, 12, S, T_enc]."""
        return self._teacher_forced("loco_decoder_forward_attn", enc_out, frames, ids, output_hidden_states, True)

    def align(self, enc_out, frames, ids, counts, heads=None, pairs=0, return_attention=False):
        """loco_decoder_align: (start i32 [B, S], end i32 [B, S], A f32 [B, S, T] or None), all on the device, nothing read back."""
        B, T, _ = enc_out.shape
        S = ids.shape[1]
        device = enc_out.device
        ws = self._grown(int(self.lib.loco_decoder_align_workspace_bytes(self.enc._handle, B, T, S)), device)
        start = torch.empty((B, S), dtype=torch.int32, device=device)
        end = torch.empty((B, S), dtype=torch.int32, device=device)
        A = torch.empty((B, S, T), dtype=torch.float32, device=device) if return_attention else None
        _lib.check(self.lib.loco_decoder_align(
            self.enc._handle, _ptr(enc_out), _ptr(frames), B, T, _ptr(ids), S, _ptr(counts), heads, pairs, _ptr(A), _ptr(start), _ptr(end),
            _ptr(ws), ws.numel(), self._stream(device)), "loco_decoder_align")
        return start, end, A

    def generate(self, enc_out, frames, max_length, return_logits=False):
        B, T, _ = enc_out.shape
        device = enc_out.device
        if B > self.max_batch():
            raise ValueError(f"generate: {B} clips exceed the decode step's limit of {self.max_batch()} rows; split the batch")
        ws = self.workspace(B, T, max_length, device)
        vocab = self.enc._decoder_vocab
        tokens = torch.empty((B, max_length), dtype=torch.int32)
        lengths = torch.empty((B,), dtype=torch.int32)
        steps = torch.zeros((max_length - 1, B, vocab), dtype=torch.float32, device=device) if return_logits else None
        n = C.c_int32(0)
        _lib.check(self.lib.loco_decoder_generate(
            self.enc._handle, _ptr(enc_out), _ptr(frames), B, T, max_length, _ptr(tokens), _ptr(lengths), C.byref(n), _ptr(steps),
            _ptr(ws), ws.numel(), self._stream(device)), "loco_decoder_generate")
        S = int(n.value)
        ids = tokens[:, :S].to(torch.long).to(device)
        self.last_lengths = lengths
        return (ids, steps[:S - 1]) if return_logits else ids


def resolve_caps(n: int, max_length=None, max_new_tokens=None):
    """One total length per utterance: ``max_length`` an int (or None) for all, or one int per utterance."""
    per_utterance = False
    if max_length is not None and max_new_tokens is None:
        try:
            max_length = operator.index(max_length)  # int, numpy integer, 0-d tensor
        except TypeError:
            per_utterance = True
    if per_utterance:
        caps = [resolve_max_length(int(v)) for v in max_length]
        if len(caps) != n:
            raise ValueError(f"max_length names {len(caps)} utterances, the batches hold {n}")
        return caps
    return [resolve_max_length(max_length, max_new_tokens)] * n


@dataclass
class PoolItem:
    """One utterance waiting for a slot: clip ``clip`` of ``enc_out`` [B, T, 768] (a packed forward's output), of which ``rows`` rows
    belong to its own reference batch; ``frames`` i32 [B] on the device.  In a pool that samples the item is hypothesis
    ``hypothesis`` of utterance ``utterance`` (the random numbers' counter), ``greedy`` = it takes the argmax all the same."""
    key: int
    enc_out: torch.Tensor
    frames: torch.Tensor
    clip: int
    rows: int
    cap: int
    utterance: int = 0
    hypothesis: int = 0
    greedy: bool = True


class DecoderPool:
    """Host side of loco_decoder_pool_*: ``slots`` decoder rows, each at its own position; a row that ends hands its slot to the next
    utterance.  Owns the workspace and the pinned poll block.  The host keeps an exact bound on every slot's position (the steps
    enqueued since its admission, at most cap - 2), so a step's launches are sized without reading the device; the device is looked at
    every ``poll_steps`` steps (8, as loco_decoder_generate does), when finished rows are collected and waiting ones admitted.
    Single caller, one stream, as DecoderRuntime.

    ``sample`` (a _lib.SampleConfig, decoder.check_sample_args) makes it the sampling pool: items are admitted through
    loco_decoder_pool_admit_samples -- the hypotheses of one utterance that fit the free slots together, the rest later -- and stepped
    through loco_decoder_pool_step_sample; scores are the model's log P of the token each step appended.

    ``beam`` (a _lib.BeamConfig, decoder.check_beam_args) makes it the beam pool: an item is one utterance and takes a group of
    ``num_beams`` slots (group g = slots g K .. g K + K - 1) through loco_decoder_pool_admit_beams, the pool is stepped through
    loco_decoder_pool_step_beam and ``collect`` yields, per finished group, the group's list of hypotheses, best first.  ``fusion``
    (an ngram.NgramLM on the pool's device, weight, token_bonus) attaches the n-gram model to the beam pool: every step then scores
    its candidates with ``weight * log P_lm + token_bonus`` added (loco_decoder_pool_attach_ngram); the pool keeps the model alive."""

    def __init__(self, encoder, slots: int, T_cap: int, S_max: int, device, poll_steps: int = 8, return_logits: bool = False,
                 return_scores: bool = False, sample=None, beam=None, trace: bool = False, fusion=None):
        self.enc, self.lib = encoder, encoder._lib
        self.fusion = fusion  # (an ngram.NgramLM on the device, weight, token_bonus) of a beam pool, or None
        assert fusion is None or beam is not None
        self.sample = sample
        self.beam = beam
        self.K = int(beam.num_beams) if beam is not None else 1
        self.trace = bool(trace) and beam is not None  # collect() then appends the log-probabilities [steps, K, V] every step chose from
        assert beam is None or (sample is None and not return_logits and int(slots) >= self.K)
        self.slots, self.T_cap, self.S_max = int(slots), int(T_cap), int(S_max)
        self.device = device
        self.poll_steps = int(poll_steps)
        self.return_logits = return_logits
        self.return_scores = return_scores  # collect() then yields 4-tuples: (..., log P of every generated token [len - 1])
        self.vocab = encoder._decoder_vocab
        if fusion is not None:
            need = int(self.lib.loco_decoder_beam_fusion_workspace_bytes(encoder._handle, self.slots, self.T_cap, self.S_max, self.K))
        elif beam is not None:
            need = int(self.lib.loco_decoder_beam_workspace_bytes(encoder._handle, self.slots, self.T_cap, self.S_max, self.K))
        else:
            need = int(self.lib.loco_decoder_pool_workspace_bytes(encoder._handle, self.slots, self.T_cap, self.S_max))
        self.workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
        self._shape = (self.slots, self.T_cap, self.S_max)
        # the limits are the library's: with need == 0 the call below names the one that was crossed
        _lib.check(self.lib.loco_decoder_pool_init(encoder._handle, *self._shape, self._ws(), need, self._stream()), "loco_decoder_pool_init")
        if fusion is not None:  # before the first admission; the handle keeps it for this workspace until the next init
            lm, weight, bonus = fusion
            _lib.check(self.lib.loco_decoder_pool_attach_ngram(encoder._handle, *self._shape, lm.handle, float(weight), float(bonus), self._ws(), need),
                       "loco_decoder_pool_attach_ngram")
        self.block = torch.zeros(4 + 2 * self.slots, dtype=torch.int32).pin_memory()
        self.tokens = torch.zeros((self.slots, self.S_max), dtype=torch.int32).pin_memory()
        self.entries = [None] * self.slots  # per slot: (item, step count at admission), None = free on the host's books
        self.steps = 0                      # steps enqueued so far
        self.waiting = []
        self._rounds = []                   # (first step, logits [k, slots, V]) of the rounds an open utterance may still need
        self._score_rounds = []             # (first step, log-probabilities [k, slots]) likewise
        self._trace_rounds = []             # (first step, log-probabilities [k, slots, V]) of a beam pool that traces
        if beam is not None:
            K, S = self.K, self.S_max
            self._fin = dict(count=torch.zeros(1, dtype=torch.int32).pin_memory(), tokens=torch.zeros((K, S), dtype=torch.int32).pin_memory(),
                             lengths=torch.zeros(K, dtype=torch.int32).pin_memory(), scores=torch.zeros(K, dtype=torch.float64).pin_memory(),
                             sums=torch.zeros(K, dtype=torch.float64).pin_memory(), tlp=torch.zeros((K, S), dtype=torch.float32).pin_memory())

    def _ws(self):
        return _ptr(self.workspace)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def submit(self, items):
        self.waiting.extend(items)

    @property
    def busy(self) -> bool:
        return bool(self.waiting) or any(e is not None for e in self.entries)

    def admit(self, slot_ids, items):
        """Clips of ONE encoder output, consecutive in it, into the given free slots."""
        n = len(items)
        first = items[0]
        assert all(it.enc_out is first.enc_out and it.clip == first.clip + i for i, it in enumerate(items))
        ids = (C.c_int32 * n)(*slot_ids)
        rows = (C.c_int32 * n)(*[it.rows for it in items])
        caps = (C.c_int32 * n)(*[it.cap for it in items])
        out = first.enc_out
        frames = first.frames[first.clip:] if first.frames is not None else None
        _lib.check(self.lib.loco_decoder_pool_admit(
            self.enc._handle, *self._shape, n, ids, _ptr(out[first.clip]), out.stride(0),
            rows, _ptr(frames), caps, self._ws(), self.workspace.numel(), self._stream()),
            "loco_decoder_pool_admit")
        for r, it in zip(slot_ids, items):
            self.entries[r] = (it, self.steps)

    def admit_samples(self, slot_ids, groups):
        """``groups``: per clip its waiting hypotheses, equally many for every clip; the clips consecutive in ONE encoder output."""
        first, copies = groups[0][0], len(groups[0])
        assert all(len(g) == copies and it.enc_out is first.enc_out and it.clip == first.clip + i and it.utterance == g[0].utterance
                   for i, g in enumerate(groups) for it in g)
        n, flat = len(groups), [it for g in groups for it in g]
        i32, u32 = lambda vs: (C.c_int32 * len(vs))(*vs), lambda vs: (C.c_uint32 * len(vs))(*vs)  # noqa: E731
        out = first.enc_out
        frames = first.frames[first.clip:] if first.frames is not None else None
        _lib.check(self.lib.loco_decoder_pool_admit_samples(
            self.enc._handle, *self._shape, n, copies, i32(slot_ids), _ptr(out[first.clip]), out.stride(0), i32([g[0].rows for g in groups]),
            _ptr(frames), i32([g[0].cap for g in groups]), u32([g[0].utterance for g in groups]), u32([it.hypothesis for it in flat]),
            i32([int(it.greedy) for it in flat]), self._ws(), self.workspace.numel(), self._stream()), "loco_decoder_pool_admit_samples")
        for r, it in zip(slot_ids, flat):
            self.entries[r] = (it, self.steps)

    def admit_beams(self, groups, items):
        """Clips of ONE encoder output, consecutive in it, into the given free groups (group g = slots g K .. g K + K - 1)."""
        n, first, K = len(items), items[0], self.K
        assert all(it.enc_out is first.enc_out and it.clip == first.clip + i for i, it in enumerate(items))
        i32 = lambda vs: (C.c_int32 * len(vs))(*vs)  # noqa: E731
        out = first.enc_out
        frames = first.frames[first.clip:] if first.frames is not None else None
        _lib.check(self.lib.loco_decoder_pool_admit_beams(
            self.enc._handle, *self._shape, C.byref(self.beam), n, i32(groups), _ptr(out[first.clip]), out.stride(0), i32([it.rows for it in items]),
            _ptr(frames), i32([it.cap for it in items]), self._ws(), self.workspace.numel(), self._stream()), "loco_decoder_pool_admit_beams")
        for g, it in zip(groups, items):
            for r in range(g * K, g * K + K):
                self.entries[r] = (it, self.steps)

    def _fill_beams(self):
        K = self.K
        free = [g for g in range(self.slots // K) if self.entries[g * K] is None]
        while free and self.waiting:
            run = [self.waiting[0]]
            while len(run) < len(free) and len(run) < len(self.waiting) and self.waiting[len(run)].enc_out is run[0].enc_out \
                    and self.waiting[len(run)].clip == run[0].clip + len(run):
                run.append(self.waiting[len(run)])
            self.admit_beams(free[:len(run)], run)
            del self.waiting[:len(run)], free[:len(run)]

    def _collect_beams(self):
        """Finished groups since the last call: [(key, hypotheses, scores f64 [n], sums of log-probabilities f64 [n], per-token
        log-probabilities [n] of f32 [len - 1], trace or None)], the n <= K entries of the group's list, best first."""
        status, lengths = self.poll()
        K, out = self.K, []
        stream = torch.cuda.current_stream(self.device)
        for g in range(self.slots // K):
            if self.entries[g * K] is None or status[g * K] != 2:
                continue
            f = self._fin
            _lib.check(self.lib.loco_decoder_pool_read_beams(self.enc._handle, *self._shape, g, _ptr(f["count"]), _ptr(f["tokens"]), _ptr(f["lengths"]),
                                                             _ptr(f["scores"]), _ptr(f["sums"]), _ptr(f["tlp"]), self._ws(), self.workspace.numel(),
                                                             self._stream()), "loco_decoder_pool_read_beams")
            stream.synchronize()
            it, s0 = self.entries[g * K]
            n = int(f["count"][0])
            lens = f["lengths"][:n].tolist()
            hyps = [f["tokens"][e, :lens[e]].to(torch.long) for e in range(n)]
            tlps = [f["tlp"][e, 1:lens[e]].clone() for e in range(n)]
            tr = None
            if self.trace:
                steps = lengths[g * K] - 1  # the steps the group took
                parts = [t[max(s0 - a, 0):s0 + steps - a, g * K:g * K + K] for a, t in self._trace_rounds if a < s0 + steps and a + t.shape[0] > s0]
                tr = torch.cat(parts).cpu()
            out.append((it.key, hyps, f["scores"][:n].clone(), f["sums"][:n].clone(), tlps, tr))
            for r in range(g * K, g * K + K):
                self.entries[r] = None
        if self.trace:
            oldest = min([s0 for e in self.entries if e is not None for _, s0 in [e]], default=self.steps)
            self._trace_rounds = [(a, t) for a, t in self._trace_rounds if a + t.shape[0] > oldest]
        return out

    def _round_beams(self):
        k = max(1, min(self.poll_steps, self.bounds()[2]))
        lp = torch.empty((k, self.slots, self.vocab), dtype=torch.float32, device=self.device) if self.trace else None
        if self.trace:
            self._trace_rounds.append((self.steps, lp))
        for j in range(k):
            max_pos, max_frames, _ = self.bounds()
            _lib.check(self.lib.loco_decoder_pool_step_beam(self.enc._handle, *self._shape, max_pos, max_frames, None, _ptr(lp[j]) if self.trace else None,
                                                            None, self._ws(), self.workspace.numel(), self._stream()), "loco_decoder_pool_step_beam")
            self.steps += 1
        return self.collect()

    def _siblings(self, at):
        """How many waiting items from ``at`` on are hypotheses of one utterance (one clip of one encoder output)."""
        w, n = self.waiting, 1
        while at + n < len(w) and w[at + n].enc_out is w[at].enc_out and w[at + n].clip == w[at].clip and w[at + n].utterance == w[at].utterance:
            n += 1
        return n

    def _fill_samples(self):
        free = [r for r in range(self.slots) if self.entries[r] is None]
        while free and self.waiting:
            head, whole = self.waiting[0], self._siblings(0)
            copies = min(whole, len(free))
            groups, taken = [self.waiting[:copies]], copies
            # further clips of the same encoder output whose hypotheses are as many and fit as well: one call, one wait for the stream
            while copies == whole and taken < len(self.waiting) and taken + copies <= len(free):
                nxt = self.waiting[taken]
                if nxt.enc_out is not head.enc_out or nxt.clip != head.clip + len(groups) or self._siblings(taken) != copies:
                    break
                groups.append(self.waiting[taken:taken + copies])
                taken += copies
            self.admit_samples(free[:taken], groups)
            del self.waiting[:taken], free[:taken]

    def _fill(self):
        if self.sample is not None:
            return self._fill_samples()
        if self.beam is not None:
            return self._fill_beams()
        free = [r for r in range(self.slots) if self.entries[r] is None]
        while free and self.waiting:
            run = [self.waiting[0]]
            while len(run) < len(free) and len(run) < len(self.waiting) and self.waiting[len(run)].enc_out is run[0].enc_out \
                    and self.waiting[len(run)].clip == run[0].clip + len(run):
                run.append(self.waiting[len(run)])
            self.admit(free[:len(run)], run)
            del self.waiting[:len(run)], free[:len(run)]

    def bounds(self):
        """(max_pos, max_frames, steps until every slot on the books has reached its cap)."""
        live = [(it, self.steps - s0) for e in self.entries if e is not None for it, s0 in [e]]
        max_pos = max(min(done, it.cap - 2) for it, done in live)
        return max_pos, max(it.rows for it, _ in live), max(it.cap - 1 - done for it, done in live)

    def step(self, logits=None, tokens=None):
        max_pos, max_frames, _ = self.bounds()
        if self.sample is not None:  # ``tokens``: i32 [slots] on the device, the token every live slot appended (-100: none)
            _lib.check(self.lib.loco_decoder_pool_step_sample(self.enc._handle, *self._shape, max_pos, max_frames, C.byref(self.sample), _ptr(logits),
                                                              _ptr(tokens), self._ws(), self.workspace.numel(), self._stream()),
                       "loco_decoder_pool_step_sample")
            self.steps += 1
            return
        _lib.check(self.lib.loco_decoder_pool_step(self.enc._handle, *self._shape, max_pos, max_frames, _ptr(logits), self._ws(), self.workspace.numel(),
                                                   self._stream()), "loco_decoder_pool_step")
        self.steps += 1

    def poll(self):
        """(status, lengths) of every slot after the work enqueued so far (waits for the stream)."""
        _lib.check(self.lib.loco_decoder_pool_poll(self.enc._handle, *self._shape, _ptr(self.block), self._ws(), self.workspace.numel(),
                                                   self._stream()), "loco_decoder_pool_poll")
        torch.cuda.current_stream(self.device).synchronize()
        b = self.block.tolist()
        return b[4:4 + self.slots], b[4 + self.slots:]

    def collect(self):
        """Finished utterances since the last call: [(key, ids LongTensor, step logits [len - 1, V] or None)], with ``return_scores``
        [(key, ids, logits or None, log-probabilities [len - 1])]; their slots are free."""
        if self.beam is not None:
            return self._collect_beams()
        status, lengths = self.poll()
        done = [r for r in range(self.slots) if self.entries[r] is not None and status[r] == 2]
        for r in done:
            _lib.check(self.lib.loco_decoder_pool_read(self.enc._handle, *self._shape, r, _ptr(self.tokens[r]), self._ws(),
                                                       self.workspace.numel(), self._stream()), "loco_decoder_pool_read")
        if done:
            torch.cuda.current_stream(self.device).synchronize()
        out = []
        for r in done:
            it, s0 = self.entries[r]
            n = lengths[r]
            lg = None
            if self.return_logits:
                parts = [t[max(s0 - g, 0):s0 + n - 1 - g, r] for g, t in self._rounds if g < s0 + n - 1 and g + t.shape[0] > s0]
                lg = torch.cat(parts) if parts else torch.empty((0, self.vocab), dtype=torch.float32, device=self.device)
            if self.return_scores:
                parts = [t[max(s0 - g, 0):s0 + n - 1 - g, r] for g, t in self._score_rounds if g < s0 + n - 1 and g + t.shape[0] > s0]
                sc = torch.cat(parts) if parts else torch.empty((0,), dtype=torch.float32, device=self.device)
                out.append((it.key, self.tokens[r, :n].to(torch.long), lg, sc))
            else:
                out.append((it.key, self.tokens[r, :n].to(torch.long), lg))
            self.entries[r] = None
        if self.return_logits or self.return_scores:
            oldest = min([s0 for e in self.entries if e is not None for _, s0 in [e]], default=self.steps)
            self._rounds = [(g, t) for g, t in self._rounds if g + t.shape[0] > oldest]
            self._score_rounds = [(g, t) for g, t in self._score_rounds if g + t.shape[0] > oldest]
        return out

    def round(self):
        """Admit what waits into the free slots, run up to ``poll_steps`` steps, collect."""
        self._fill()
        if not any(e is not None for e in self.entries):
            return []
        if self.beam is not None:
            return self._round_beams()
        k = max(1, min(self.poll_steps, self.bounds()[2]))
        want = self.return_logits or self.return_scores
        lg = torch.empty((k, self.slots, self.vocab), dtype=torch.float32, device=self.device) if want else None
        if self.return_logits:
            self._rounds.append((self.steps, lg))
        first = self.steps
        drawn = self.sample is not None and self.return_scores
        tok = torch.empty((k, self.slots), dtype=torch.int32, device=self.device) if drawn else None
        for j in range(k):
            self.step(lg[j] if lg is not None else None, *((tok[j],) if drawn else ()))
        if self.return_scores:  # the round's block in one launch: every row against its own argmax, the token the step appended
            # (a pool that samples: against the token it appended, on the raw logits -- the model's log P, not the warped distribution's)
            self._score_rounds.append((first, score_logits(self.lib, lg, tok, k, self.slots, reduce=False)[0]))
        return self.collect()

    def drain(self):
        out = []
        while self.busy:
            out += self.round()
        return out
