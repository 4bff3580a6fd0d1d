"""``SpeechT5ForSpeechToTextMI355X``: HuggingFace's speech-to-text model over the speech encoder (encoder.py) and, when decoder
weights are loaded, the text decoder (decoder.py) -- ``forward(decoder_input_ids= / labels=)``, ``generate``, ``score``, ``align`` and
their corpus forms ``generate_many`` / ``score_many`` / ``align_many``, which share one walk over the corpus (``corpus_packs``);
``sample`` / ``sample_many`` draw n-best lists in ``generate_many``'s slot pool and ``mbr_many`` picks from them the hypothesis of
least expected edit distance to the others (metrics.py); ``transcribe_long`` cuts a recording at pauses
(segment.py) and hands the segments to ``generate_many`` / ``align_many``."""
from __future__ import annotations

import itertools
import re
from typing import Optional

import torch
from torch import nn

from . import checkpoint_map
from . import decoder as dec
from . import segment as seg
from .encoder import SpeechT5EncoderWithSpeechPrenetMI355X
from .holders import _Ref
from .synth import LAYERS


def corpus_packs(what, sizes, pack, labels, check_row):
    """The walk over a labelled corpus that ``score_many`` and ``align_many`` (``what``: the name their messages carry) share, on the
    host alone: ``sizes`` is the utterance count of every batch, ``labels`` one 1-D tensor of token ids per utterance in input order,
    ``check_row`` what the caller asks of such a row (it returns the row as a host LongTensor).  Returns, per pack of ``pack`` batches
    (a batch without utterances is skipped), (the batches' indices, the slice of their utterances, those utterances' rows as one
    LongTensor [n, S], each padded with -100 to the pack's longest).  ValueError before anything is built: label rows that do not
    number the utterances, ``pack`` < 1, a row that is not a 1-D tensor or that ``check_row`` refuses."""
    if len(labels) != sum(sizes):
        raise ValueError(f"{what}: {len(labels)} label rows for {sum(sizes)} utterances")
    if int(pack) < 1:
        raise ValueError("pack must be >= 1")
    hosts = []
    for u, lab in enumerate(labels):
        if not torch.is_tensor(lab) or lab.dim() != 1:
            raise ValueError(f"{what}: labels[{u}] must be a 1-D tensor of token ids")
        hosts.append(check_row(lab))
    first = [0] + list(itertools.accumulate(sizes))  # first[i]: the first utterance of batch i
    kept = [i for i, n in enumerate(sizes) if n]
    packs = []
    for g0 in range(0, len(kept), int(pack)):
        idx = kept[g0:g0 + int(pack)]
        us = slice(first[idx[0]], first[idx[-1] + 1])
        rows = hosts[us]
        lab = torch.full((len(rows), max(int(r.shape[0]) for r in rows)), dec.IGNORE_INDEX, dtype=torch.long)
        for i, r in enumerate(rows):
            lab[i, :r.shape[0]] = r
        packs.append((idx, us, lab))
    return packs


class _SpeechT5Core(nn.Module):
    def __init__(self, encoder, decoder=None):
        super().__init__()
        self.encoder = encoder
        if decoder is not None:
            self.decoder = decoder


class SpeechT5ForSpeechToTextMI355X(nn.Module):
    """HF's SpeechT5ForSpeechToText as the reference uses it: ``.speecht5.encoder`` (the embedding path), and -- when decoder
    weights are loaded (``decoder_layers > 0``) -- ``.speecht5.decoder`` / ``.text_decoder_postnet`` with ``forward(...,
    decoder_input_ids=...)`` and greedy ``generate`` (decoder.py).  An encoder-only model is exactly what it was."""

    def __init__(self, layers: int = LAYERS, precision: str = "f16x3", decoder_layers: int = 0, vocab_size: Optional[int] = None):
        super().__init__()
        encoder = SpeechT5EncoderWithSpeechPrenetMI355X(layers, precision)
        decoder = None
        if decoder_layers:
            ref = _Ref()
            ref.obj = encoder
            decoder = dec.SpeechT5DecoderWithTextPrenetMI355X(ref, decoder_layers, vocab_size or dec.TEXT_VOCAB)
            postnet = dec.SpeechT5TextDecoderPostnetMI355X(ref, vocab_size or dec.TEXT_VOCAB)
            encoder._extra_weights = [("decoder.", decoder), ("text_decoder_postnet.", postnet)]
            encoder._decoder_layers = decoder_layers
            encoder._decoder_vocab = vocab_size or dec.TEXT_VOCAB
            self._decoder_runtime = dec.DecoderRuntime(encoder)
        self.speecht5 = _SpeechT5Core(encoder, decoder)
        if decoder is not None:
            self.text_decoder_postnet = postnet
        self.eval()

    @property
    def has_decoder(self) -> bool:
        return hasattr(self, "text_decoder_postnet")

    def _require_decoder(self, what: str):
        if not self.has_decoder:
            why = getattr(self, "_no_decoder_reason", None)
            raise RuntimeError(f"{what} needs the decoder, and this model was loaded without one: speecht5.decoder.* and "
                               "text_decoder_postnet.lm_head.weight are missing (from_pretrained on a full speech-to-text checkpoint, or "
                               "from_state_dicts(..., decoder_state_dict=, postnet_state_dict=))" + (f" -- {why}" if why else ""))

    def _encode(self, input_values, attention_mask):
        out = self.speecht5.encoder(input_values=input_values, attention_mask=attention_mask)
        return out.last_hidden_state, self.speecht5.encoder.last_frames

    def _encode_with_attentions(self, input_values, attention_mask):
        out = self.speecht5.encoder(input_values=input_values, attention_mask=attention_mask, output_attentions=True)
        return out.last_hidden_state, self.speecht5.encoder.last_frames, out.attentions

    def _encode_pack(self, group):
        """One pack of reference batches through the packed encoder: (out [B, T, 768], spans, frames i32 [B], ticket).  The ticket owns
        the packed input: a caller holds it until its next pack, so that the block returns to the allocator when it always has."""
        enc = self.speecht5.encoder
        ticket = enc.forward_packed_async(group)
        ticket.result()
        out, spans = ticket.packed_output()
        return out, spans, enc.last_frames, ticket

    @torch.no_grad()
    def forward(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                decoder_input_ids: Optional[torch.Tensor] = None, output_hidden_states: Optional[bool] = None,
                labels: Optional[torch.Tensor] = None, output_attentions: Optional[bool] = None, **kwargs):
        """``model(**audios, decoder_input_ids=ids)``: teacher-forced logits [B, S, vocab] and ``encoder_last_hidden_state``
        (``output_hidden_states=True``: also the 7 ``decoder_hidden_states``).  Causal self-attention over the ids as given (no
        decoder attention mask, as in the reference's calls); cross-attention over each clip's valid encoder frames.

        ``labels`` [B, S] (token ids, -100 = not counted): also ``loss``, HF's mean cross-entropy over the counted labels, and
        ``token_logprobs`` [B, S].  Without ``decoder_input_ids`` the decoder reads the labels shifted right (decoder.shift_tokens_right),
        as HF does; with both, the given ids are read and the loss is taken against ``labels``.

        ``output_attentions=True``: also ``decoder_attentions`` (6 x [B, 12, S, S], key j visible to query i iff j <= i),
        ``cross_attentions`` (6 x [B, 12, S, T_enc], key j visible iff it is a valid frame of its clip) and ``encoder_attentions`` (the
        encoder's own flag), fp32, masked entries exactly 0; formed by launches of their own (csrc/decoder_probs.hip), so logits
        and hidden states are the same bits with and without the flag."""
        for k in kwargs:
            if k in ("decoder_attention_mask", "past_key_values", "encoder_outputs", "use_cache"):
                raise NotImplementedError(f"forward({k}=...) is not implemented")
            raise TypeError(f"forward() got an unexpected keyword argument '{k}'")
        self._require_decoder("forward(labels=...)" if labels is not None and decoder_input_ids is None else "forward(decoder_input_ids=...)")
        if decoder_input_ids is None and labels is None:
            raise ValueError("You have to specify `decoder_input_ids` (for embeddings alone call model.speecht5.encoder)")
        targets = None
        if labels is not None:  # on the host, before any launch
            host = dec.check_labels(labels, int(input_values.shape[0]), self.speecht5.encoder._decoder_vocab,
                                    decoder_input_ids.shape if decoder_input_ids is not None else None)
            if decoder_input_ids is None:
                decoder_input_ids = dec.shift_tokens_right(host)
            targets = host.to(torch.int32)
        enc_attn = self_attn = cross_attn = None
        if output_attentions:
            enc_out, frames, enc_attn = self._encode_with_attentions(input_values, attention_mask)
        else:
            enc_out, frames = self._encode(input_values, attention_mask)
        if decoder_input_ids.dim() != 2 or decoder_input_ids.shape[0] != enc_out.shape[0]:
            raise ValueError(f"decoder_input_ids must be [batch, tokens] with batch {enc_out.shape[0]}, got {tuple(decoder_input_ids.shape)}")
        ids = decoder_input_ids.to(device=enc_out.device, dtype=torch.int32).contiguous()
        with torch.cuda.device(enc_out.device):
            if output_attentions:
                logits, hidden, self_attn, cross_attn = self._decoder_runtime.forward_attn(enc_out, frames, ids, bool(output_hidden_states))
            else:
                logits, hidden = self._decoder_runtime.forward(enc_out, frames, ids, bool(output_hidden_states))
            loss = logprobs = None
            if targets is not None:
                logprobs, _, _, loss, _ = dec.score_logits(self.speecht5.encoder._lib, logits, targets.to(enc_out.device).contiguous(), *ids.shape)
        return dec.Seq2SeqLMOutput(logits=logits, encoder_last_hidden_state=enc_out, decoder_hidden_states=hidden, loss=loss, token_logprobs=logprobs,
                                   decoder_attentions=self_attn, cross_attentions=cross_attn, encoder_attentions=enc_attn)

    @torch.no_grad()
    def align(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
              alignment_heads=None, return_attention: bool = False):
        """Where in the audio each token of the transcripts ``labels`` [B, S] was spoken: a decoder.TokenAlignment with ``start_frames`` /
        ``end_frames`` i32 [B, S] (encoder frames, end exclusive, -1 where the label is -100) and ``start_times`` / ``end_times`` in seconds
        (frames x 320 / 16000, the conv stack's stride; its receptive-field offset is ignored).  -100 may only pad the end of a row.

        One teacher-forced pass on the labels shifted right; the mean of the cross-attention probabilities over ``alignment_heads``
        ((layer, head) pairs; None = all 72) is the soft alignment A [B, S, T_enc] (``return_attention=True`` hands it out), and a
        monotone DTW over -A from (0, 0) to (n_b - 1, frames_b - 1) -- on the device, in double -- gives every token its frames."""
        self._require_decoder("align()")
        if labels is None:
            raise ValueError("align() needs labels")
        enc = self.speecht5.encoder
        host = dec.check_labels(labels, int(input_values.shape[0]), enc._decoder_vocab)
        counts = dec.alignment_counts(host)
        heads, pairs = dec.check_alignment_heads(alignment_heads, enc._decoder_layers)
        enc_out, frames = self._encode(input_values, attention_mask)
        return self._align_encoded(enc_out, frames, host, counts, heads, pairs, return_attention)

    def _align_encoded(self, enc_out, frames, labels_host, counts, heads, pairs, return_attention):
        device = enc_out.device
        ids = dec.shift_tokens_right(labels_host).to(device=device, dtype=torch.int32).contiguous()
        with torch.cuda.device(device):
            start, end, A = self._decoder_runtime.align(enc_out, frames, ids, counts.to(device).contiguous(), heads, pairs, return_attention)
            seconds = lambda f: torch.where(f < 0, -1.0, f.to(torch.float32) * dec.FRAME_SECONDS).to(torch.float32)  # noqa: E731
            return dec.TokenAlignment(start_frames=start, end_frames=end, start_times=seconds(start), end_times=seconds(end), attention=A)

    @torch.no_grad()
    def align_many(self, batches, labels, pack: int = 8, alignment_heads=None, return_attention: bool = False):
        """Token timestamps of a corpus, built the way ``score_many`` is: ``batches`` is what ``generate_many`` takes, ``labels`` one
        1-D LongTensor per utterance in input order (no -100 needed: each row is padded to its pack's longest).  The batches are
        encoded ``pack`` at a time through ``forward_packed``; each pack's clips go through ONE ``align`` pass on the packed output and
        its frame counts.  Returns a list, in input order, of decoder.TokenAlignment whose fields are the utterance's own 1-D slices
        (``attention`` [len, T of its pack]).  An utterance's A is that of ``align`` on its own batch up to the fp32 summation order
        of the packed encoder and of the decoder's products; its path is the DTW of that A."""
        self._require_decoder("align_many()")
        enc = self.speecht5.encoder
        batches, labels = list(batches), list(labels)

        def check_row(lab):
            host = dec.check_labels(lab[None], 1, enc._decoder_vocab)[0]
            dec.alignment_counts(host[None])
            return host

        packs = corpus_packs("align_many", [int(b["input_values"].shape[0]) for b in batches], pack, labels, check_row)
        heads, pairs = dec.check_alignment_heads(alignment_heads, enc._decoder_layers)
        results = []
        for idx, us, lab in packs:
            out, _, frames, ticket = self._encode_pack([batches[i] for i in idx])
            al = self._align_encoded(out, frames, lab, dec.alignment_counts(lab), heads, pairs, return_attention)
            for i, u in enumerate(range(us.start, us.stop)):
                k = int(labels[u].shape[0])
                results.append(dec.TokenAlignment(start_frames=al.start_frames[i, :k], end_frames=al.end_frames[i, :k], start_times=al.start_times[i, :k],
                                                  end_times=al.end_times[i, :k], attention=al.attention[i, :k] if al.attention is not None else None))
        return results

    @torch.no_grad()
    def score(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None):
        """How likely the model finds the transcripts ``labels`` [B, S] (-100 = not counted) for these clips: decoder.TranscriptScores
        with ``token_logprobs`` [B, S], ``sequence_logprob`` [B], ``tokens`` [B] and ``loss`` -- ``forward(labels=...)``'s pass, without
        handing the logits out."""
        self._require_decoder("score()")
        if labels is None:
            raise ValueError("score() needs labels")
        host = dec.check_labels(labels, int(input_values.shape[0]), self.speecht5.encoder._decoder_vocab)
        enc_out, frames = self._encode(input_values, attention_mask)
        return self._score_encoded(enc_out, frames, host)

    def _score_encoded(self, enc_out, frames, labels_host):
        device = enc_out.device
        ids = dec.shift_tokens_right(labels_host).to(device=device, dtype=torch.int32).contiguous()
        with torch.cuda.device(device):
            logits, _ = self._decoder_runtime.forward(enc_out, frames, ids)
            lp, seq, cnt, loss, _ = dec.score_logits(self.speecht5.encoder._lib, logits, labels_host.to(device=device, dtype=torch.int32).contiguous(),
                                                     *ids.shape)
        return dec.TranscriptScores(token_logprobs=lp, sequence_logprob=seq, tokens=cnt, loss=loss)

    @torch.no_grad()
    def score_many(self, batches, labels, pack: int = 8):
        """Scores of a corpus: ``batches`` is what ``generate_many`` takes, ``labels`` one 1-D LongTensor per utterance in input order.
        The batches are encoded ``pack`` at a time through ``forward_packed``; each pack's clips go through ONE teacher-forced
        decoder pass on the packed output and its frame counts, their labels padded with -100 to the pack's longest, and are scored
        in one launch.  Returns a list, in input order, of (``token_logprobs`` 1-D of the utterance's own length, its sum 0-d), both
        on the device.  An utterance's scores are those of ``score`` on its own batch up to the fp32 summation order of the packed
        encoder and of the decoder's products, whatever ``pack`` is; the scoring kernel itself adds nothing to that (a row's
        log-probability is a function of the row's logits alone)."""
        self._require_decoder("score_many()")
        vocab = self.speecht5.encoder._decoder_vocab
        batches, labels = list(batches), list(labels)
        packs = corpus_packs("score_many", [int(b["input_values"].shape[0]) for b in batches], pack, labels,
                             lambda lab: dec.check_labels(lab[None], 1, vocab)[0])
        results = []
        for idx, us, lab in packs:
            out, _, frames, ticket = self._encode_pack([batches[i] for i in idx])
            sc = self._score_encoded(out, frames, lab)
            for i, u in enumerate(range(us.start, us.stop)):
                results.append((sc.token_logprobs[i, :labels[u].shape[0]], sc.sequence_logprob[i]))
        return results

    @torch.no_grad()
    def generate(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, max_length: Optional[int] = None,
                 max_new_tokens: Optional[int] = None, return_logits: bool = False, return_dict_in_generate: bool = False,
                 output_scores: bool = False, **kwargs):
        """Greedy search as HF's ``generate`` runs it for this model: LongTensor [B, S] starting with decoder_start_token_id 2, a
        row that has emitted </s> (2) is filled with <pad> (1), S = the longest row or ``max_length`` (total, start token included;
        ``max_new_tokens`` counts the tokens after it).  ``return_logits=True``: also the logits [S - 1, B, vocab] each step chose from.

        ``return_dict_in_generate=True``: a decoder.GreedySearchOutput whose ``sequences`` are those ids; with ``output_scores=True``
        it also carries ``scores`` (the S - 1 step logits [B, vocab]), ``token_logprobs`` [B, S - 1] and ``sequence_logprobs`` [B].
        ``output_scores`` alone changes nothing, as in HF."""
        dec.check_generate_kwargs(kwargs)
        self._require_decoder("generate()")
        n = dec.resolve_max_length(max_length, max_new_tokens)
        enc_out, frames = self._encode(input_values, attention_mask)
        with_scores = bool(return_dict_in_generate) and bool(output_scores)
        with torch.cuda.device(enc_out.device):
            rt = self._decoder_runtime
            res = rt.generate(enc_out, frames, n, return_logits or with_scores)
            if not return_dict_in_generate:
                return res
            ids, steps = res if (return_logits or with_scores) else (res, None)
            out = dec.GreedySearchOutput(sequences=ids)
            if with_scores:
                B, S = ids.shape
                # targets: the returned ids, -100 from each row's length on (the host holds ids' lengths already)
                cols = torch.arange(1, S)[None, :]
                targets = torch.where(cols < rt.last_lengths[:, None].long(), ids[:, 1:].cpu(), torch.tensor(dec.IGNORE_INDEX)).to(torch.int32)
                by_row = steps.permute(1, 0, 2).contiguous()  # [B, S - 1, V]: a row's steps form one sequence
                lp, seq, _, _, _ = dec.score_logits(self.speecht5.encoder._lib, by_row, targets.to(enc_out.device).contiguous(), B, S - 1)
                out.scores, out.token_logprobs, out.sequence_logprobs = tuple(steps[t] for t in range(S - 1)), lp, seq
            return (out, steps) if return_logits else out

    @torch.no_grad()
    def generate_many(self, batches, max_length=None, max_new_tokens: Optional[int] = None, slots: int = 64, return_logits: bool = False,
                      pack: int = 8, return_scores: bool = False, **kwargs):
        """Greedy transcripts of a corpus: ``batches`` is what ``pack_batches`` takes (reference batches of ``input_values`` /
        ``attention_mask``), ``max_length`` an int or one int per utterance (total length, start token included).  The batches are
        encoded ``pack`` at a time through ``forward_packed`` -- every clip keeps its own batch's padded length -- and decoded in a
        pool of ``slots`` decoder rows in which a row that ends hands its slot to the next utterance (decoder.DecoderPool).

        Returns a list, in input order, of 1-D LongTensors (host): <s> ... up to and including </s>, or the utterance's cap of tokens
        for a row that never ended -- row u of ``generate(**batch_k, max_length=cap_u)`` without its trailing <pad>, up to the fp32
        summation order of the packed encoder and of the attention's key splits.  An utterance's result does not depend on the
        utterances decoded beside it.  ``return_logits=True``: (ids, logits) with one [len - 1, vocab] device tensor per utterance.
        ``return_scores=True``: (ids, scores) with one [len - 1] device tensor per utterance, the log-probability of every generated
        token (both: (ids, logits, scores))."""
        dec.check_generate_kwargs(kwargs)
        self._require_decoder("generate_many()")
        batches, total, caps = self._corpus_args("generate_many", batches, max_length, max_new_tokens, slots, pack)
        extras = int(bool(return_logits)) + int(bool(return_scores))
        if total == 0:
            return ([],) * (1 + extras) if extras else []
        results = self._decode_corpus(batches, caps, slots, pack, return_logits, return_scores)
        out = [[results[k][0] for k in range(total)]]
        if return_logits:
            out.append([results[k][1] for k in range(total)])
        if return_scores:
            out.append([results[k][2] for k in range(total)])
        return tuple(out) if extras else out[0]

    def _corpus_args(self, what, batches, max_length, max_new_tokens, slots, pack):
        """What ``generate_many`` and ``sample_many`` (``what``: the name their messages carry) ask of their arguments before anything is
        built: (the batches as a list, their utterances in all, every utterance's cap of tokens)."""
        batches = list(batches)
        total = sum(int(b["input_values"].shape[0]) for b in batches)
        caps = dec.resolve_caps(total, max_length, max_new_tokens)
        if int(pack) < 1:
            raise ValueError("pack must be >= 1")
        most = int(self.speecht5.encoder._lib.loco_decoder_max_batch())
        if not 1 <= int(slots) <= most:
            raise ValueError(f"{what}: slots = {slots} is outside 1 .. {most}, the decode step's limit of rows")
        return batches, total, caps

    def _decode_corpus(self, batches, caps, slots, pack, return_logits, return_scores, copies=1, sample=None, greedy_first=False, first_utterance=0,
                       beam=None, trace=False, fusion=None):
        """The walk ``generate_many`` and ``sample_many`` share over checked arguments: encode ``pack`` batches at a time, decode in one
        pool.  {utterance * copies + hypothesis: [ids, logits or None, scores when asked for]}; ``sample`` (a _lib.SampleConfig) makes
        the pool draw ``copies`` hypotheses per utterance, of which hypothesis 0 is the argmax path with ``greedy_first``.  ``beam`` (a
        _lib.BeamConfig) makes it the beam pool: {utterance: what DecoderPool.collect yields per group}; ``fusion`` (lm, weight, bonus)
        attaches an n-gram model to that pool."""
        total = len(caps)
        enc = self.speecht5.encoder
        lib = enc._lib
        device = enc._device()
        T_cap = max(int(lib.loco_output_frames(int(b["input_values"].shape[1]))) for b in batches if b["input_values"].shape[0])
        if T_cap < 1:
            raise ValueError("input shorter than one encoder frame (400 samples)")
        pool = None
        results, u, nxt = {}, 0, 0
        batches = [b for b in batches if b["input_values"].shape[0]]
        with torch.cuda.device(device):
            while nxt < len(batches) or (pool is not None and pool.busy):
                if nxt < len(batches) and (pool is None or len(pool.waiting) < int(slots)):
                    out, spans, frames, ticket = self._encode_pack(batches[nxt:nxt + int(pack)])
                    nxt += int(pack)
                    if pool is None:  # after the first forward: the handle exists and carries the decoder's weights
                        rows = total * copies * (int(beam.num_beams) if beam is not None else 1)
                        pool = dec.DecoderPool(enc, min(int(slots), rows), T_cap, max(caps), device,
                                               return_logits=return_logits, return_scores=return_scores, sample=sample, beam=beam, trace=trace,
                                               fusion=(fusion[0].to(device),) + tuple(fusion[1:]) if fusion is not None else None)
                    items = []
                    for b0, nb, t in spans:
                        for c in range(b0, b0 + nb):
                            for h in range(copies):
                                items.append(dec.PoolItem(key=u * copies + h, enc_out=out, frames=frames, clip=c, rows=t, cap=caps[u],
                                                          utterance=first_utterance + u, hypothesis=h,
                                                          greedy=sample is None or (bool(greedy_first) and h == 0)))
                            u += 1
                    pool.submit(items)
                    continue
                for k, *rest in pool.round():
                    results[k] = rest
        return results

    @torch.no_grad()
    def sample_many(self, batches, num_return_sequences: int = 1, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed=None,
                    greedy_first: bool = False, max_length=None, max_new_tokens: Optional[int] = None, slots: int = 64, pack: int = 8,
                    return_logits: bool = False, return_scores: bool = False, first_utterance: int = 0):
        """``num_return_sequences`` sampled transcripts of every utterance of a corpus -- an n-best list for ``score_many`` to rescore,
        or for confidence by agreement (``mbr_many``, metrics.mbr_select).  ``batches``, ``max_length`` (an int or one per utterance), ``slots`` and ``pack`` are
        ``generate_many``'s; the N hypotheses of an utterance are N rows of the same slot pool.  Each token is drawn on the device
        (csrc/decoder_sample.hip): logits / ``temperature``, ``top_k`` (0 = off; ties at the threshold survive), ``top_p`` (1 = off;
        HF's TopPLogitsWarper, equal logits kept or dropped together), then one draw from the softmax of what is kept.  The uniform
        behind a draw is a Philox4x32-10 block keyed by ``seed`` with the counter (utterance, hypothesis, token index): a hypothesis
        does not depend on the hypotheses decoded beside it, on ``slots`` or on the admission order, bit for bit.  The utterance index
        is ``first_utterance`` + the utterance's position in the call.  ``seed=None`` draws a 63-bit seed from torch's default CPU
        generator, so ``torch.manual_seed`` makes a call reproducible; the seed used is ``.seed`` of the result.
        ``greedy_first=True``: hypothesis 0 is the argmax path, ``generate_many``'s transcript.

        Returns ``hyps`` with ``hyps[u][h]`` a 1-D LongTensor (host), <s> ... </s> or the cap.  ``return_logits=True``: (hyps, logits)
        with ``logits[u][h]`` [len - 1, vocab] on the device, the raw logits each token was drawn from; ``return_scores=True``: (hyps,
        scores) with ``scores[u][h]`` [len - 1] on the device, the model's log P of every token (of the unwarped distribution); both:
        (hyps, logits, scores)."""
        self._require_decoder("sample_many()")
        n, config = dec.check_sample_args(num_return_sequences, temperature, top_k, top_p, seed)
        batches, total, caps = self._corpus_args("sample_many", batches, max_length, max_new_tokens, slots, pack)
        if not 0 <= int(first_utterance) <= 2 ** 32 - 1 - total:
            raise ValueError(f"sample_many: first_utterance = {first_utterance} leaves no room for {total} utterances below 2^32")
        results = self._decode_corpus(batches, caps, slots, pack, return_logits, return_scores, copies=n, sample=config,
                                      greedy_first=greedy_first, first_utterance=int(first_utterance)) if total else {}
        out = []
        for field in range(1 + int(bool(return_logits)) + int(bool(return_scores))):
            src = field if field == 0 or return_logits else 2  # a round's result: [ids, logits or None, scores when asked for]
            out.append([[results[u * n + h][src] for h in range(n)] for u in range(total)])
        hyps = dec.SampledHypotheses(out[0])
        hyps.seed = int(config.seed)
        if len(out) == 1:
            return hyps
        res = dec.SampledResults([hyps] + out[1:])
        res.seed = hyps.seed
        return res

    @torch.no_grad()
    def beam_search_many(self, batches, num_beams: int = 4, num_return_sequences: Optional[int] = None, length_penalty: float = 1.0,
                         early_stopping=False, max_length=None, max_new_tokens: Optional[int] = None, slots: int = 64, pack: int = 8,
                         return_scores: bool = False, return_step_logprobs: bool = False, lm=None, lm_weight: float = 0.0, lm_bonus: float = 0.0):
        """Beam search over a corpus, HF's ``generate(num_beams=K, num_return_sequences=N, length_penalty=, early_stopping=)``:
        ``batches``, ``max_length`` (an int or one per utterance), ``slots`` and ``pack`` are ``generate_many``'s.  An utterance takes a
        group of ``num_beams`` rows of the slot pool (``slots >= num_beams``; ``slots // num_beams`` utterances decode together); the
        selection, the finished lists and the reordering of the self-attention cache by parent beam run on the device
        (csrc/decoder_beam.hip).  The rule is HF's ``_beam_search`` with scores carried in float64 and ties broken towards the lower
        (beam, token) index; an utterance's result does not depend on ``slots``, the admission order or its neighbours, bit for bit.

        Returns ``hyps`` with ``hyps[u][h]`` a 1-D LongTensor (host), best first, ``num_return_sequences`` (None = 1) per utterance,
        ``hyps.sequence_scores[u]`` float64 [N] (HF's ``sequences_scores``) and ``hyps.sequence_logprobs[u]`` float64 [N].
        ``return_scores=True``: (hyps, scores) with ``scores[u][h]`` float32 [len - 1], the log-probability of every token.
        ``return_step_logprobs=True``: also ``hyps.step_logprobs[u]`` float32 [steps, num_beams, vocab] (host), the log-softmax rows
        every step of the utterance chose from -- what a restatement of the rule needs to replay the search.

        Shallow fusion: ``lm`` (an ngram.NgramLM over the decoder's ids; None = the search as it always was) adds
        ``lm_weight * log P_lm(token | hypothesis so far) + lm_bonus`` to every candidate's score on the device (include/loco_asr.h
        states the rule).  ``sequence_scores`` and ``sequence_logprobs`` are then the FUSED values, ``scores`` / ``step_logprobs`` stay
        the acoustic model's, and ``hyps.lm_logprobs[u]`` float64 [N] holds every hypothesis' n-gram log-probability, so that
        ``sequence_logprobs = sum(scores) + lm_weight * lm_logprobs + lm_bonus * (len - 1)`` up to rounding."""
        self._require_decoder("beam_search_many()")
        k, n, config = dec.check_beam_args(num_beams, num_return_sequences, length_penalty, early_stopping,
                                           vocab=self.speecht5.encoder._decoder_vocab)
        fusion = dec.check_fusion_args(lm, lm_weight, lm_bonus, vocab=self.speecht5.encoder._decoder_vocab)
        batches, total, caps = self._corpus_args("beam_search_many", batches, max_length, max_new_tokens, slots, pack)
        if int(slots) < k:
            raise ValueError(f"beam_search_many: slots = {slots} is below num_beams = {k}, the rows of one utterance")
        results = self._decode_corpus(batches, caps, slots, pack, False, False, beam=config, trace=return_step_logprobs, fusion=fusion) if total else {}
        hyps = dec.BeamHypotheses([list(results[u][0][:n]) for u in range(total)])
        hyps.sequence_scores = [results[u][1][:n] for u in range(total)]
        hyps.sequence_logprobs = [results[u][2][:n] for u in range(total)]
        if fusion is not None and total:  # one scoring launch over every hypothesis returned
            flat = iter(fusion[0].token_logprobs([h for per in hyps for h in per]))
            hyps.lm_logprobs = [torch.stack([next(flat).sum() for _ in per]) if len(per) else torch.zeros(0, dtype=torch.float64) for per in hyps]
        elif fusion is not None:
            hyps.lm_logprobs = []
        if return_step_logprobs:
            hyps.step_logprobs = [results[u][4] for u in range(total)]
        if not return_scores:
            return hyps
        return hyps, [list(results[u][3][:n]) for u in range(total)]

    @torch.no_grad()
    def beam_search(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, num_beams: int = 4,
                    num_return_sequences: Optional[int] = None, length_penalty: float = 1.0, early_stopping=False,
                    max_length: Optional[int] = None, max_new_tokens: Optional[int] = None, slots: int = 64, lm=None, lm_weight: float = 0.0,
                    lm_bonus: float = 0.0):
        """``beam_search_many`` for one batch, in HF's ``num_return_sequences`` layout: a decoder.BeamSearchOutput whose ``sequences``
        are LongTensor [B * N, S] on the inputs' device -- clip b's hypotheses, best first, in rows b * N .. b * N + N - 1, <pad> (1)
        after the end, S the longest row -- with ``sequences_scores`` float64 [B * N], ``token_logprobs`` [B * N, S - 1] (exactly 0 at
        the <pad> columns) and ``sequence_logprobs`` float64 [B * N].  ``lm``, ``lm_weight``, ``lm_bonus``: ``beam_search_many``'s shallow
        fusion; the scores are then the fused ones and ``lm_logprobs`` float64 [B * N] is filled."""
        self._require_decoder("beam_search()")
        if attention_mask is None:
            attention_mask = torch.ones(input_values.shape, dtype=torch.int32, device=input_values.device)
        hyps, scores = self.beam_search_many([dict(input_values=input_values, attention_mask=attention_mask)], num_beams=num_beams,
                                             num_return_sequences=num_return_sequences, length_penalty=length_penalty,
                                             early_stopping=early_stopping, max_length=dec.resolve_max_length(max_length, max_new_tokens),
                                             slots=slots, pack=1, return_scores=True, lm=lm, lm_weight=lm_weight, lm_bonus=lm_bonus)
        rows = [h for per in hyps for h in per]
        device = input_values.device
        S = max((int(r.shape[0]) for r in rows), default=1)
        seqs = torch.full((len(rows), S), dec.PAD_TOKEN_ID, dtype=torch.long)
        tlp = torch.zeros((len(rows), max(S - 1, 0)), dtype=torch.float32)
        for i, (r, l) in enumerate(zip(rows, [l for per in scores for l in per])):
            seqs[i, :r.shape[0]] = r
            tlp[i, :l.shape[0]] = l
        cat = lambda per: torch.cat(list(per)) if len(rows) else torch.zeros(0, dtype=torch.float64)  # noqa: E731
        return dec.BeamSearchOutput(sequences=seqs.to(device), sequences_scores=cat(hyps.sequence_scores).to(device), token_logprobs=tlp.to(device),
                                    sequence_logprobs=cat(hyps.sequence_logprobs).to(device),
                                    lm_logprobs=cat(hyps.lm_logprobs).to(device) if hyps.lm_logprobs is not None else None)

    @torch.no_grad()
    def mbr_many(self, batches, num_return_sequences: int = 8, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed=None,
                 greedy_first: bool = False, max_length=None, max_new_tokens: Optional[int] = None, slots: int = 64, pack: int = 8,
                 unit: str = "token", delimiter_id: Optional[int] = None, weights=None, return_scores: bool = False, first_utterance: int = 0):
        """Minimum-Bayes-risk transcripts of a corpus: ``sample_many`` with the same arguments and the same seed contract, then
        ``metrics.mbr_select`` over every utterance's ``num_return_sequences`` hypotheses -- the one of least expected edit distance
        to the others (``unit``, ``delimiter_id``: what is compared; ``weights``: None = every sample counts 1, ``"logprob"`` = the
        softmax of the hypotheses' sequence log-probabilities within the list).  Ties go to the lowest index, so with ``greedy_first``
        the greedy transcript wins them.  Because a hypothesis does not depend on ``slots`` and the distances are integers, the same
        seed gives the same choice at any ``slots``.

        Returns a metrics.MbrTranscripts: ``ids[u]`` the chosen hypothesis (a 1-D LongTensor, host), ``best[u]`` its index, ``risk[u]``
        the risk of every hypothesis of the utterance (float64, device), ``hypotheses`` what ``sample_many`` returned, ``seed`` the seed
        used, and with ``return_scores`` ``scores[u][h]``, the hypotheses' per-token log-probabilities."""
        from . import metrics
        if weights is not None and weights != "logprob":
            raise ValueError(f"mbr_many: weights = {weights!r} is not None or 'logprob'")
        need_scores = bool(return_scores) or weights == "logprob"
        if unit == "word" and delimiter_id is None:  # refused before anything is decoded
            raise ValueError("mbr_many: unit='word' needs delimiter_id, the id of the checkpoint's word-boundary token (there is no default)")
        if unit not in ("token", "word"):
            raise ValueError(f"mbr_many: unit = {unit!r} is not 'token' or 'word'")
        res = self.sample_many(batches, num_return_sequences=num_return_sequences, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                               greedy_first=greedy_first, max_length=max_length, max_new_tokens=max_new_tokens, slots=slots, pack=pack,
                               return_scores=need_scores, first_utterance=first_utterance)
        hyps, scores = res if need_scores else (res, None)
        if not len(hyps):
            return metrics.MbrTranscripts(ids=[], best=[], risk=[], hypotheses=hyps, seed=hyps.seed, scores=scores if return_scores else None)
        sel = metrics.mbr_select(hyps, weights=weights, unit=unit, delimiter_id=delimiter_id, scores=scores if weights == "logprob" else None)
        best = sel.best.cpu().tolist()  # the one read-back
        return metrics.MbrTranscripts(ids=[per[b] for per, b in zip(hyps, best)], best=best, risk=sel.risk, hypotheses=hyps, seed=hyps.seed,
                                      scores=scores if return_scores else None)

    @torch.no_grad()
    def sample(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, num_return_sequences: int = 1,
               temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed=None, greedy_first: bool = False,
               max_length: Optional[int] = None, max_new_tokens: Optional[int] = None, slots: int = 64, return_scores: bool = False):
        """``sample_many`` for one batch, in HF's ``num_return_sequences`` layout: a decoder.SampleOutput whose ``sequences`` are
        LongTensor [B * N, S] on the inputs' device -- clip b's hypotheses in rows b * N .. b * N + N - 1, <pad> (1) after </s>, S the
        longest row -- and whose ``seed`` is the seed used.  The rows are ``sample_many``'s hypotheses for the same seed (utterance
        index = the clip's row in the batch): the same pool, the same kernel.  ``return_scores=True``: also ``token_logprobs``
        [B * N, S - 1], exactly 0 at the <pad> columns, and ``sequence_logprobs`` [B * N], as decoder.GreedySearchOutput's."""
        self._require_decoder("sample()")
        if attention_mask is None:
            attention_mask = torch.ones(input_values.shape, dtype=torch.int32, device=input_values.device)
        res = self.sample_many([dict(input_values=input_values, attention_mask=attention_mask)], num_return_sequences=num_return_sequences,
                               temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, greedy_first=greedy_first,
                               max_length=dec.resolve_max_length(max_length, max_new_tokens), slots=slots, pack=1, return_logits=bool(return_scores))
        hyps, logits = res if return_scores else (res, None)
        rows = [h for per in hyps for h in per]
        device = input_values.device
        S = max((int(r.shape[0]) for r in rows), default=1)
        seqs = torch.full((len(rows), S), dec.PAD_TOKEN_ID, dtype=torch.long)
        for i, r in enumerate(rows):
            seqs[i, :r.shape[0]] = r
        out = dec.SampleOutput(sequences=seqs.to(device), seed=res.seed)
        if return_scores and rows and S > 1:
            # one scoring launch over [B * N, S - 1, V]: the rows' own step logits, the <pad> columns not counted
            flat = [l for per in logits for l in per]
            V = self.speecht5.encoder._decoder_vocab
            block = torch.zeros((len(rows), S - 1, V), dtype=torch.float32, device=flat[0].device)
            targets = torch.full((len(rows), S - 1), dec.IGNORE_INDEX, dtype=torch.int32)
            for i, (r, l) in enumerate(zip(rows, flat)):
                block[i, :l.shape[0]] = l
                targets[i, :r.shape[0] - 1] = r[1:].to(torch.int32)
            with torch.cuda.device(block.device):
                lp, seq, _, _, _ = dec.score_logits(self.speecht5.encoder._lib, block, targets.to(block.device).contiguous(), len(rows), S - 1)
            out.token_logprobs, out.sequence_logprobs = lp, seq
        return out

    @torch.no_grad()
    def transcribe_long(self, waveform: torch.Tensor, vad=None, max_length: Optional[int] = None, slots: int = 64, pack: int = 8,
                        return_scores: bool = False, timestamps: bool = False, do_normalize: bool = False, num_beams: Optional[int] = None,
                        length_penalty: float = 1.0, early_stopping=False, lm=None, lm_weight: float = 0.0, lm_bonus: float = 0.0):
        """A transcript of a whole recording: ``waveform`` is a 1-D 16 kHz CUDA tensor of any length from one encoder frame on.  It is
        cut at pauses on the device (segment.segment; ``vad``: None, a segment.VadParams or a dict of its fields), and every segment is
        a batch of ONE clip -- ``input_values = waveform[s:e][None]``, mask all ones -- so its padded length is its own and GroupNorm
        sees nothing of its neighbours: a segment's transcript depends on the segment's samples alone.  The batches go through
        ``generate_many`` in time order (``max_length`` None = 450, the decoder's positions; ``slots``, ``pack`` as there) and, with
        ``timestamps``, through ``align_many``; nothing else is computed here.

        Returns a segment.LongTranscript whose ``segments[k]`` carries ``start_s`` / ``end_s``, ``ids``, with ``return_scores``
        ``token_logprobs`` (device), ``logprob`` and ``avg_logprob``, and with ``timestamps`` ``token_times`` [len - 1, 2] in
        recording time (``align_many``'s times plus ``start_s``).  ``do_normalize``: each segment is normalised on its own.
        ``num_beams`` (None: greedy, as ever): every segment's ids are the best beam of ``beam_search_many`` with ``length_penalty`` and
        ``early_stopping``, its scores that beam's.  ``lm``, ``lm_weight``, ``lm_bonus`` (with ``num_beams``) are ``beam_search_many``'s
        shallow fusion; the segments' ``token_logprobs`` stay the acoustic model's."""
        def cut(params):
            segs = seg.segment(waveform, params)
            wave = waveform.to(torch.float32)
            return segs, [segs.start_samples, segs.end_samples], lambda s, e: wave[s:e]
        return self._transcribe_cut("transcribe_long()", cut, vad, max_length, slots, pack, return_scores, timestamps, do_normalize,
                                    (num_beams, length_penalty, early_stopping), (lm, lm_weight, lm_bonus))

    @torch.no_grad()
    def transcribe_channels(self, waveforms: torch.Tensor, crosstalk_db: float = seg.DEFAULT_CROSSTALK_DB, vad=None, max_length: Optional[int] = None,
                            slots: int = 64, pack: int = 8, return_scores: bool = False, timestamps: bool = False, do_normalize: bool = False,
                            num_beams: Optional[int] = None, length_penalty: float = 1.0, early_stopping=False, lm=None, lm_weight: float = 0.0,
                            lm_bonus: float = 0.0):
        """``transcribe_long`` for a recording with one speaker per channel (a two-channel telephone call): ``waveforms`` is a
        [channels, samples] 16 kHz CUDA tensor.  Every channel is cut at its own pauses (segment.segment_channels; a frame in which
        another channel is louder by more than ``crosstalk_db`` is not speech), and every segment of every channel is a batch of ONE
        clip, ``waveforms[c, s:e][None]``: all of them go through one ``generate_many`` (and one ``align_many`` with ``timestamps``), so
        a segment's ids depend on its own samples alone.

        Returns a segment.LongTranscript in (start, channel) order; its segments also carry ``channel`` and ``overlap_s``, and its
        ``threshold_db`` is a list with one threshold per channel."""
        def cut(params):
            segs = seg.segment_channels(waveforms, crosstalk_db, params)
            waves = waveforms.to(torch.float32)
            return (segs, [segs.start_samples, segs.end_samples, segs.channel.to(torch.int64), segs.overlap_frames.to(torch.int64)],
                    lambda s, e, c, _: waves[c, s:e])
        return self._transcribe_cut("transcribe_channels()", cut, vad, max_length, slots, pack, return_scores, timestamps, do_normalize,
                                    (num_beams, length_penalty, early_stopping), (lm, lm_weight, lm_bonus))

    def _transcribe_cut(self, what, cut, vad, max_length, slots, pack, return_scores, timestamps, do_normalize, beam=(None, 1.0, False),
                        fusion=(None, 0.0, 0.0)):
        """``transcribe_long`` and ``transcribe_channels`` (``what``) but for the cut itself.  ``cut(params)`` cuts the recording and
        returns (the Segments / ChannelSegments, the per-segment table as device columns -- start samples, end samples and, per channel,
        channel and overlap frames --, a callable that takes a row of that table to the segment's samples).  Everything else is here: the
        one-clip batches, ``generate_many`` (or, with ``beam`` = (num_beams, length_penalty, early_stopping) and num_beams not None,
        the best beam of ``beam_search_many``), the score sums, ``align_many``, the LongTranscript."""
        self._require_decoder(what)
        if beam[0] is not None:  # refused before the recording is cut
            dec.check_beam_args(beam[0], 1, beam[1], beam[2], vocab=self.speecht5.encoder._decoder_vocab)
            dec.check_fusion_args(*fusion, vocab=self.speecht5.encoder._decoder_vocab)
        elif fusion[0] is not None:
            raise ValueError(f"{what}: lm= needs num_beams=: shallow fusion is part of beam search")
        params = seg.resolve_params(vad)
        cap = dec.resolve_max_length(dec.MAX_TEXT_POSITIONS if max_length is None else max_length)
        segs, columns, clip = cut(params)
        duration = segs.samples / seg.SAMPLE_RATE
        if segs.count == 0:
            return seg.LongTranscript(segments=[], duration_s=duration, threshold_db=segs.threshold_db)
        from .feature_extractor import SpeechT5FeatureExtractorMI355X
        fe = SpeechT5FeatureExtractorMI355X(do_normalize=do_normalize)
        table = list(zip(*torch.stack(columns).cpu().tolist()))  # one read-back: a row per segment
        batches = [fe(audio=[clip(*row)], sampling_rate=seg.SAMPLE_RATE) for row in table]
        if beam[0] is None:
            rows = self.generate_many(batches, max_length=cap, slots=slots, pack=pack, return_scores=return_scores)
            ids, scores = rows if return_scores else (rows, None)
        else:
            hyps, per_token = self.beam_search_many(batches, num_beams=beam[0], length_penalty=beam[1], early_stopping=beam[2], max_length=cap,
                                                    slots=slots, pack=pack, return_scores=True, lm=fusion[0], lm_weight=fusion[1], lm_bonus=fusion[2])
            device = batches[0]["input_values"].device
            ids, scores = [per[0] for per in hyps], [per[0].to(device) for per in per_token] if return_scores else None
        out = []
        for (s, e, *rest), r in zip(table, ids):
            out.append(seg.LongSegment(start_s=s / seg.SAMPLE_RATE, end_s=e / seg.SAMPLE_RATE, ids=r))
            if rest:
                out[-1].channel, out[-1].overlap_s = rest[0], rest[1] / seg.FRAME_RATE
        if return_scores:
            sums = [float(v) for v in torch.stack([t.double().sum() for t in scores]).cpu().tolist()]  # one read-back
            for o, t, v in zip(out, scores, sums):
                o.token_logprobs, o.logprob, o.avg_logprob = t, v, v / max(int(t.shape[0]), 1)
        if timestamps:
            for o, al in zip(out, self.align_many(batches, [r[1:] for r in ids], pack=pack)):
                o.token_times = torch.stack([al.start_times, al.end_times], dim=1).cpu() + o.start_s
        return seg.LongTranscript(segments=out, duration_s=duration, threshold_db=segs.threshold_db)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, precision: str = "f16x3", **_unused):
        """``SpeechT5ForSpeechToText.from_pretrained(...)`` of the fine-tuned script (…finetuned…py:95) for a checkpoint ON
        DISK: a directory holding ``model.safetensors`` / ``pytorch_model.bin`` (or their sharded index), one such file, or a hub
        name that is already in the local HuggingFace cache -- nothing is ever downloaded.  Keeps ``speecht5.encoder.prenet.*``
        and ``speecht5.encoder.wrapped_encoder.*`` (either spelling of the weight-normed positional conv) and, when the file has
        them, ``speecht5.decoder.*`` and ``text_decoder_postnet.*`` (the tied embedding / lm_head pair may be present once); takes
        the layer counts from the keys, and fails BY NAME on anything the encoder needs and the file lacks
        (load_state_dict(strict=True)).  The decoder is kept only when the file holds a COMPLETE one (checkpoint_map.decoder_problem):
        a file with the encoder and stray or partial decoder tensors gives the encoder-only model it always gave, and ``generate`` /
        ``decoder_input_ids`` then raise with the name of the first decoder tensor that is missing or misshapen."""
        checkpoint_map.check_hf_config(str(pretrained_model_name_or_path))
        pre, enc = checkpoint_map.load_hf_checkpoint(str(pretrained_model_name_or_path))
        ids = [int(m_.group(1)) for m_ in (re.match(r"layers\.(\d+)\.", k) for k in enc) if m_]
        if not ids:
            raise KeyError(f"{pretrained_model_name_or_path}: no speecht5.encoder.wrapped_encoder.layers.N.* tensors")
        dec_sd, post_sd = checkpoint_map.load_hf_decoder(str(pretrained_model_name_or_path))
        problem = checkpoint_map.decoder_problem(dec_sd, post_sd)
        if problem is not None:  # no (complete) decoder in the file: the encoder-only model this call has always returned
            model = cls.from_state_dicts(pre, enc, layers=max(ids) + 1, precision=precision)
            model._no_decoder_reason = f"{pretrained_model_name_or_path}: {problem}"
            return model
        known = {"prenet.embed_tokens.weight"} | {"wrapped_decoder." + n for l in range(64) for n, _, _ in dec.decoder_layer_keys(l)}
        dec_sd = {k: v for k, v in dec_sd.items() if k in known}  # e.g. a stray wrapped_decoder.layer_norm of another architecture
        return cls.from_state_dicts(pre, enc, layers=max(ids) + 1, precision=precision, decoder_state_dict=dec_sd,
                                    postnet_state_dict={k: v for k, v in post_sd.items() if k == "lm_head.weight"})

    @classmethod
    def from_state_dicts(cls, prenet_state_dict, encoder_state_dict, layers: int = LAYERS, precision: str = "f16x3",
                         decoder_state_dict=None, postnet_state_dict=None):
        """What the base script does after from_pretrained (…base…py:98-100), minus the hub download.  With ``decoder_state_dict``
        (keys ``prenet.embed_tokens.weight``, ``wrapped_decoder.layers.N.*``) and / or ``postnet_state_dict`` (``lm_head.weight``)
        the model also decodes; of the tied pair embed_tokens / lm_head one may be absent (it is taken from the other)."""
        dec_layers, vocab = 0, None
        if decoder_state_dict is not None or postnet_state_dict is not None:
            decoder_state_dict = dict(decoder_state_dict or {})
            postnet_state_dict = dict(postnet_state_dict or {})
            emb, head = decoder_state_dict.get("prenet.embed_tokens.weight"), postnet_state_dict.get("lm_head.weight")
            if emb is None and head is None:
                raise KeyError("decoder weights without prenet.embed_tokens.weight or lm_head.weight (the tied pair: one of them is needed)")
            decoder_state_dict.setdefault("prenet.embed_tokens.weight", head)
            postnet_state_dict.setdefault("lm_head.weight", emb)
            ids = [int(m_.group(1)) for m_ in (re.match(r"wrapped_decoder\.layers\.(\d+)\.", k) for k in decoder_state_dict) if m_]
            if not ids:
                raise KeyError("decoder_state_dict: no wrapped_decoder.layers.N.* tensors")
            dec_layers, vocab = max(ids) + 1, int(decoder_state_dict["prenet.embed_tokens.weight"].shape[0])
        model = cls(layers, precision, decoder_layers=dec_layers, vocab_size=vocab)
        model.speecht5.encoder.wrapped_encoder.load_state_dict(encoder_state_dict)
        model.speecht5.encoder.prenet.load_state_dict(prenet_state_dict)
        if dec_layers:
            as_t = lambda d: {k: (v if torch.is_tensor(v) else torch.as_tensor(v)) for k, v in d.items()}  # noqa: E731
            model.speecht5.decoder.load_state_dict(as_t(decoder_state_dict))
            model.text_decoder_postnet.load_state_dict(as_t(postnet_state_dict))
        return model
