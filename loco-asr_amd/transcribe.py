"""Greedy transcription CLI: ``python -m loco-asr_amd.transcribe`` writes one JSON line per utterance, {"id", "token_ids"} (and
"text" when a SentencePiece model for ``--tokenizer`` is found ON DISK; nothing is ever fetched).  ``--scores`` adds "logprob", the sum of
the generated tokens' log-probabilities, and "avg_logprob", that sum divided by their number -- a confidence to filter lines by.
``--timestamps`` adds "token_times", one [start_s, end_s] pair per generated token (the ids after the start token, up to the row's own
end; the <pad> columns behind it get none): ``align`` / ``align_many`` on the generated ids, the mean cross-attention and a monotone DTW.

Utterances go through the model in the reference's pairs (batch_size 2, corpus order), encoder + ``generate`` per pair.  With
``--slots N`` the pairs are encoded ``--pack G`` at a time and decoded in a pool of N decoder rows in which a finished row hands its
slot to the next utterance (``generate_many``); the lines written are the same.  ``--nbest N`` (with ``--slots``) adds "nbest": N
sampled transcripts of the utterance (``sample_many``: ``--temperature``, ``--top-k``, ``--top-p``, ``--seed``), each {"ids", "logprob",
"avg_logprob"} (and "text"), sorted by "logprob", best first.  The line's other fields are then hypothesis 0: the greedy transcript only
with ``--greedy-first``, a sampled one otherwise; ``--select mbr`` makes them the hypothesis of least expected edit distance to the
list's others instead (metrics.mbr_select) and adds "mbr_risk" to every "nbest" entry.  ``--beams K`` (with ``--slots`` >= K) decodes by
beam search instead (``beam_search_many``: ``--length-penalty``, ``--early-stopping false|true|never``): the line's own fields are the
best beam, ``--nbest N`` (N <= K) then lists the N best beams in the search's order, each with "score" (HF's ``sequences_scores``) beside
"logprob" and "avg_logprob", and ``--select mbr`` works on that list; the sampling flags do not go with it.  ``--ngram lm.arpa`` (with ``--beams``; ``--lm-weight W``, default 1, ``--lm-bonus B``,
default 0) fuses a character n-gram model over the decoder's ids into the search (ngram.py): "logprob" and "score" are then the fused
values, and ``--scores`` adds "lm_logprob" to the line and to every "nbest" entry.  ``--ref FILE`` (Kaldi ``utt_id text``; needs a
tokenizer on disk) or ``--ref-ids FILE`` (``utt_id id id ...``) adds "errors": {"cer", "wer"?, "sub", "del", "ins", "ref_len"} to every
line that has a reference and writes the corpus ``%CER`` / ``%WER`` lines to stderr.  No data parallelism.  Inputs, as extract.py takes them: a SLURP split (``--data-path slurp --split devel``: the
same reader, headset recording first; .wav / .flac, other rates resampled on the device), audio files named on the command line, or
``--synthetic N`` seeded clips; weights: ``--pretrained DIR`` (a HuggingFace speech-to-text checkpoint directory with the decoder)
or ``--random-init`` (the deterministic synthetic weights).

``--long FILE...`` transcribes whole recordings (a 10-minute call, a podcast): each file is cut at pauses on the device (segment.py:
``--max-segment-s``, ``--min-silence-s``, ``--vad-margin-db``, ``--no-trim``) and its segments are decoded in the slot pool
(``transcribe_long``; ``--slots`` defaults to 64).  One JSON line per recording: {"id", "duration_s", "threshold_db", "segments":
[{"start_s", "end_s", "token_ids", "text"?, "logprob"?, "avg_logprob"?, "token_times"?}], "text"?}, the times in recording time.
``--channels split`` (default ``mix``: the channels are averaged, as ever) cuts and decodes every channel of a file on its own -- one
speaker per channel, as in a two-channel telephone call (``transcribe_channels``; ``--crosstalk-db X``: a frame is not speech when
another channel is louder by more than X dB, default 15).  Segments then also carry "channel" ("A", "B", ... by index) and "overlap_s",
they come in (start, channel) order, and "threshold_db" is a list per channel.  ``--kaldi-text FILE`` (with ``split`` and a tokenizer
on disk) also writes one Kaldi line per segment with text, ``<rec>-<A|B>-<%06d start>-<%06d end> <text>`` in centiseconds: eval_ppl's input.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import metrics, synth
from .audio_io import load_audio_16k, load_audio_channels_16k
from .decoder import EOS_TOKEN_ID, IGNORE_INDEX, PAD_TOKEN_ID, check_beam_args, check_sample_args
from .extract import read_slurp_split
from .feature_extractor import SpeechT5FeatureExtractorMI355X
from .lm import read_key_text
from .score_errors import rec_key
from .segment import resolve_params
from .speech_to_text import SpeechT5ForSpeechToTextMI355X


def load_tokenizer(path):
    """A SentencePiece processor for ``path`` (an ``spm_char.model`` file or a directory holding one), or None."""
    if not path:
        return None
    cand = [path, os.path.join(path, "spm_char.model")]
    spm_file = next((c for c in cand if os.path.isfile(c)), None)
    if spm_file is None:
        return None
    try:
        import sentencepiece as spm
    except ImportError:
        return None
    return spm.SentencePieceProcessor(model_file=spm_file)


def strip_special(ids):
    out = []
    for t in ids[1:]:
        if t == EOS_TOKEN_ID:
            break
        if t != PAD_TOKEN_ID:
            out.append(int(t))
    return out


def row_length(row):
    """Tokens of a generated row up to and including its </s> (the start token counts; the whole row when it never ended)."""
    for i, t in enumerate(row[1:], 1):
        if t == EOS_TOKEN_ID:
            return i + 1
    return len(row)


def timestamp_labels(rows):
    """The labels ``align`` reads for generated rows: the ids after the start token, the <pad> columns behind a row's end as -100."""
    width = max(len(r) for r in rows) - 1
    lab = torch.full((len(rows), max(width, 1)), IGNORE_INDEX, dtype=torch.long)
    for i, r in enumerate(rows):
        n = row_length(r) - 1
        lab[i, :n] = torch.tensor(r[1:1 + n], dtype=torch.long)
    return lab


def rounded_pairs(pairs):
    """"token_times" as written: [[start_s, end_s], ...] of (start, end) pairs, to a tenth of a millisecond."""
    return [[round(a, 4), round(b, 4)] for a, b in pairs]


def token_times(al, i, n):
    """[[start_s, end_s], ...] of the first n tokens of row i of a TokenAlignment (one read-back)."""
    return rounded_pairs(zip(al.start_times[i, :n].cpu().tolist(), al.end_times[i, :n].cpu().tolist()))


def gather_items(args):
    """[(utterance id, audio path or None, samples for a synthetic clip)] in corpus order; exactly one input source."""
    sources = [bool(args.split), bool(args.files), args.synthetic > 0]
    if sum(sources) != 1:
        raise SystemExit("give exactly one input: --split (with --data-path), audio FILES, or --synthetic N")
    if args.split:
        return [(str(it[0]), it[2], 0) for it in read_slurp_split(args.data_path, args.split)]
    if args.files:
        return [(os.path.splitext(os.path.basename(f))[0], f, 0) for f in args.files]
    lengths = synth.mixed_lengths(args.synthetic, int(args.synthetic_seconds * synth.SAMPLE_RATE))
    return [(f"synthetic-{i:06d}", None, n) for i, n in enumerate(lengths)]


def load_batch(items, first_index, processor, device):
    """One reference batch: decoded (or synthesised) clips, padded to the longest and masked as the feature extractor does."""
    clips = [synth.clip(first_index + i, n) if path is None else load_audio_16k(path, device=device) for i, (_, path, n) in enumerate(items)]
    if any(torch.is_tensor(c) and c.is_cuda for c in clips):  # a resampled clip lives on the device: pad the whole batch there
        clips = [c if torch.is_tensor(c) else torch.from_numpy(np.asarray(c)).to(device) for c in clips]
    return processor(audio=clips, sampling_rate=synth.SAMPLE_RATE, return_tensors="pt", padding="longest")


def build_model(args):
    if args.pretrained:
        model = SpeechT5ForSpeechToTextMI355X.from_pretrained(args.pretrained, precision=args.precision)
    elif args.random_init:
        t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
        pre, enc = synth.split_state_dict(synth.encoder_state_dict(0))
        dec, post = synth.split_decoder_state_dict(synth.decoder_state_dict(0))
        model = SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), precision=args.precision, decoder_state_dict=t(dec),
                                                                postnet_state_dict=t(post))
    else:
        raise SystemExit("give --pretrained DIR or --random-init")
    if not model.has_decoder:
        raise SystemExit(f"{args.pretrained}: the checkpoint has no speecht5.decoder.* / text_decoder_postnet.* tensors: nothing to transcribe with")
    return model.to("cuda")


def channel_name(index):
    """"A", "B", ... by channel index, as Fisher's data preparation names channel 1 and channel 2."""
    return chr(ord("A") + int(index))


def kaldi_rec_id(path):
    """The recording id of a file: its base name without the extension, ``-`` and whitespace replaced by ``_`` -- eval_ppl takes an
    utterance id up to its first ``-`` as the recording (score_errors.rec_key, which maps --long's JSON ids the same way)."""
    return rec_key(os.path.splitext(os.path.basename(path))[0])


def kaldi_text_lines(rec_id, segments):
    """Kaldi ``utt_id text`` lines of one recording, ``<rec>-<A|B|..>-<%06d start>-<%06d end> <text>`` with start and end in
    centiseconds: start = start_samples // 160, end = ceil(end_samples / 160), integers both.  ``segments``: (channel index,
    start_samples, end_samples, text) in the order to write; a segment whose text is empty (or blank) is left out.  A pure function."""
    lines = []
    for channel, start, end, text in segments:
        text = " ".join(str(text).split())
        if text:
            lines.append(f"{rec_id}-{channel_name(channel)}-{int(start) // 160:06d}-{-(-int(end) // 160):06d} {text}")
    return lines


def pair_rate(table, n):
    """(sub + del + ins) / ref_len of pair n of a metrics.count_table; None for an empty reference -- JSON has no nan."""
    return (table[0][n] + table[1][n] + table[2][n]) / table[3][n] if table[3][n] else None


class RefScorer:
    """``--ref`` / ``--ref-ids``: every line's "errors" and the corpus totals (metrics.edit_counts: minimum cost, then most correct
    symbols).  ``refs``: {utt_id: text} or, with ``ids_mode``, {utt_id: [id, ...]}.  Text is compared by character ("cer"; runs of
    whitespace count as one blank) and by word ("wer"); ids by token ("cer" alone; <s>, </s> and <pad> dropped on both sides).  The
    line's sub / del / ins / ref_len are the "cer" comparison's.  An utterance without a reference is named once and not counted."""

    def __init__(self, refs, ids_mode):
        self.refs, self.ids_mode = refs, bool(ids_mode)
        self.missing, self.scored = [], 0
        self.totals = {"CER": [0, 0, 0, 0]} if ids_mode else {"CER": [0, 0, 0, 0], "WER": [0, 0, 0, 0]}

    def errors(self, uids, rows, texts):
        """One "errors" dict per row (None without a reference): one device pass per unit for the whole call."""
        for uid in uids:
            if uid not in self.refs and uid not in self.missing:
                self.missing.append(uid)
                print(f"no reference for {uid}: not counted", file=sys.stderr)
        have = [k for k, uid in enumerate(uids) if uid in self.refs]
        out = [None] * len(uids)
        if not have:
            return out
        if self.ids_mode:  # one device pass and one read-back per unit (metrics.count_table)
            tables = {"CER": metrics.count_table([metrics.strip_specials(self.refs[uids[k]]) for k in have],
                                                 [metrics.strip_specials(rows[k]) for k in have])}
        else:
            refs, hyps = [self.refs[uids[k]] for k in have], [texts[k] for k in have]
            tables = {"CER": metrics.count_table(refs, hyps, "char"), "WER": metrics.count_table(refs, hyps, "word")}
        for name, table in tables.items():
            for f in range(4):
                self.totals[name][f] += sum(table[f])
        for n, k in enumerate(have):
            t = tables["CER"]
            rec = {"cer": pair_rate(t, n)}
            if "WER" in tables:
                rec["wer"] = pair_rate(tables["WER"], n)
            rec.update({"sub": t[0][n], "del": t[1][n], "ins": t[2][n], "ref_len": t[3][n]})
            out[k] = rec
        self.scored += len(have)
        return out

    def report(self):
        """The corpus totals as Kaldi lines, then how many utterances were compared and how many had no reference."""
        lines = [metrics.format_kaldi_line(name, *tot) for name, tot in self.totals.items()]
        return lines + [f"scored {self.scored} utterances, {len(self.missing)} without a reference"]


def load_references(args, tok):
    """The RefScorer of ``--ref`` / ``--ref-ids``, or None; SystemExit naming what is missing."""
    if args.ref_ids is not None:
        refs = {}
        for uid, text in read_key_text(args.ref_ids).items():
            try:
                refs[uid] = [int(t) for t in text.split()]
            except ValueError:
                raise SystemExit(f"--ref-ids {args.ref_ids}: the line of {uid} is not 'utt_id id id ...'")
        return RefScorer(refs, ids_mode=True)
    if args.ref is None:
        return None
    if tok is None:
        raise SystemExit("--ref needs a tokenizer found on disk (--tokenizer: an spm_char.model file or a directory holding one): it compares text; "
                         "--ref-ids compares token ids without one")
    if args.ref:
        return RefScorer(dict(read_key_text(args.ref)), ids_mode=False)
    if not args.split:
        raise SystemExit("--ref without a FILE needs --split: the references are then the SLURP sentences of the split")
    return RefScorer({str(it[0]): str(it[1]) for it in read_slurp_split(args.data_path, args.split)}, ids_mode=False)


# ---- records: what a line of --out holds ---------------------------------------------------------------------------------------
@dataclass
class Line:
    """One utterance on its way to --out.  ``ids``: its generated row without padding; ``logprob``: (the sum of the generated tokens'
    log-probabilities, how many the decode path counts as generated); ``times``: its "token_times"; ``nbest``: the records of its
    hypotheses; ``errors``: its "errors"; ``lm_logprob`` (--ngram with --scores): its n-gram log-probability.  A field that is None is not
    written."""
    uid: str
    ids: list
    logprob: Optional[tuple] = None
    times: Optional[list] = None
    nbest: Optional[list] = None
    errors: Optional[dict] = None
    lm_logprob: Optional[float] = None


def token_fields(tok, ids, logprob=None, avg_logprob=None, times=None):
    """What an utterance and a segment share, in the order written: token_ids, text?, logprob?, avg_logprob?, token_times?.  The
    values are the caller's (a segment's average is ``transcribe_long``'s, an utterance's its decode path's); "text" is ``ids`` read by
    the tokenizer, when one was found."""
    rec = {"token_ids": ids}
    if tok is not None:
        rec["text"] = tok.decode(strip_special(ids))
    if logprob is not None:
        rec["logprob"], rec["avg_logprob"] = logprob, avg_logprob
    if times is not None:
        rec["token_times"] = times
    return rec


def utterance_record(line, tok, width=0):
    """The JSON object of a Line: id, the token fields, nbest?, errors?; the row <pad>-ded up to ``width`` tokens."""
    total, n = line.logprob if line.logprob is not None else (None, None)
    rec = {"id": line.uid}
    rec.update(token_fields(tok, line.ids + [PAD_TOKEN_ID] * (width - len(line.ids)), total, None if total is None else total / n, line.times))
    if line.lm_logprob is not None:
        rec["lm_logprob"] = line.lm_logprob
    if line.nbest is not None:
        rec["nbest"] = line.nbest
    if line.errors is not None:
        rec["errors"] = line.errors
    return rec


def nbest_records(hyps, sums, tok, risk=None, beam_scores=None, lm_sums=None):
    """One utterance's "nbest": its hypotheses (1-D id tensors) by log-probability ``sums[h]``, best first, ties by hypothesis index;
    ``risk``: per hypothesis its "mbr_risk".  ``beam_scores`` (--beams): the hypotheses stay in the search's order, best score first,
    and every entry carries its "score"; ``lm_sums`` (--ngram with --scores): per hypothesis its "lm_logprob"."""
    recs = []
    for h in (range(len(hyps)) if beam_scores is not None else sorted(range(len(hyps)), key=lambda h: (-sums[h], h))):
        row = hyps[h].tolist()
        rec = {"ids": row}
        if beam_scores is not None:
            rec["score"] = beam_scores[h]
        rec.update({"logprob": sums[h], "avg_logprob": sums[h] / (len(row) - 1)})
        if lm_sums is not None:
            rec["lm_logprob"] = lm_sums[h]
        if tok is not None:
            rec["text"] = tok.decode(strip_special(row))
        if risk is not None:
            rec["mbr_risk"] = risk[h]
        recs.append(rec)
    return recs


def segment_record(sg, tok, split, scores, timestamps):
    """The JSON object of a LongSegment: channel?, start_s, end_s, overlap_s?, then the token fields (``split``: --channels split)."""
    rec = {"channel": channel_name(sg.channel)} if split else {}
    rec.update(start_s=round(sg.start_s, 4), end_s=round(sg.end_s, 4))
    if split:
        rec["overlap_s"] = round(sg.overlap_s, 4)
    rec.update(token_fields(tok, sg.ids.tolist(), sg.logprob if scores else None, sg.avg_logprob if scores else None,
                            rounded_pairs(sg.token_times.tolist()) if timestamps else None))
    return rec


def finite_or_none(t):
    """JSON has no infinities."""
    return t if math.isfinite(t) else None


def recording_record(rec_id, res, tok, split, scores, timestamps):
    """The JSON object of a LongTranscript: id, duration_s, threshold_db (a list per channel with ``split``), segments, text?."""
    rec = {"id": rec_id, "duration_s": round(res.duration_s, 4),
           "threshold_db": [finite_or_none(t) for t in res.threshold_db] if split else finite_or_none(res.threshold_db),
           "segments": [segment_record(sg, tok, split, scores, timestamps) for sg in res.segments]}
    if tok is not None:
        rec["text"] = " ".join(one["text"] for one in rec["segments"])
    return rec


def write_lines(fh, batch, tok):
    """One reference batch of Lines to --out, as ``generate`` returns a batch: every row <pad>-ded up to the batch's longest."""
    width = max(len(line.ids) for line in batch)
    for line in batch:
        fh.write(json.dumps(utterance_record(line, tok, width)) + "\n")


def write_recording(fh, kh, path, res, run):
    """One recording's line to --out and, with --kaldi-text, its segments' lines there (a tokenizer is on disk then)."""
    args, split = run.args, run.args.channels == "split"
    rec = recording_record(os.path.splitext(os.path.basename(path))[0], res, run.tok, split, args.scores, args.timestamps)
    fh.write(json.dumps(rec) + "\n")
    if kh is not None:
        rows = [(sg.channel, round(sg.start_s * 16000), round(sg.end_s * 16000), one["text"]) for sg, one in zip(res.segments, rec["segments"])]
        kh.writelines(line + "\n" for line in kaldi_text_lines(kaldi_rec_id(path), rows))


@contextlib.contextmanager
def open_outputs(args):
    """(the handle of --out, the handle of --kaldi-text or None), both closed on the way out -- stdout excepted."""
    with contextlib.ExitStack() as stack:
        fh = sys.stdout if args.out == "-" else stack.enter_context(open(args.out, "w"))
        kh = stack.enter_context(open(args.kaldi_text, "w", encoding="utf-8")) if args.kaldi_text else None
        yield fh, kh


# ---- flags: every refusal that needs no device, before a model is built --------------------------------------------------------------
def check_args(args, ap):
    """Refuses what the parsed arguments alone show to be wrong; without ``--long`` (whose own checks are ``check_long_args``) also
    resolves ``--seed``: one seed for the whole corpus, whatever the windows."""
    if args.select is not None and not args.nbest:
        ap.error("--select needs --nbest: it chooses among the hypotheses of the n-best list")
    if args.ref is not None and args.ref_ids is not None:
        ap.error("give --ref or --ref-ids, not both")
    sampling = (("--temperature", args.temperature != ap.get_default("temperature")), ("--top-k", args.top_k != ap.get_default("top_k")),
                ("--top-p", args.top_p != ap.get_default("top_p")), ("--seed", args.seed is not None), ("--greedy-first", args.greedy_first))
    if args.beams is not None:
        for flag, given in sampling:
            if given:
                ap.error(f"{flag} does not go with --beams: beam search draws nothing")
        if args.long:
            ap.error("--beams does not go with --long")
    else:
        for flag, v in (("--length-penalty", args.length_penalty), ("--early-stopping", args.early_stopping), ("--ngram", args.ngram)):
            if v is not None:
                ap.error(f"{flag} needs --beams")
    for flag, v in (("--lm-weight", args.lm_weight), ("--lm-bonus", args.lm_bonus)):
        if v is not None and args.ngram is None:
            ap.error(f"{flag} needs --ngram")
        if v is not None and not math.isfinite(v):
            ap.error(f"{flag} {v} must be finite")
    if args.long:
        return
    for flag, v in (("--max-segment-s", args.max_segment_s), ("--min-silence-s", args.min_silence_s), ("--vad-margin-db", args.vad_margin_db),
                    ("--no-trim", args.no_trim or None), ("--channels", args.channels), ("--crosstalk-db", args.crosstalk_db),
                    ("--kaldi-text", args.kaldi_text)):
        if v is not None:
            raise SystemExit(f"{flag} needs --long")
    if args.batch_size < 1:
        raise SystemExit("--batch-size must be >= 1")
    if args.slots < 0 or args.pack < 1:
        raise SystemExit("--slots must be >= 0 and --pack >= 1")
    if args.nbest and not args.slots:
        raise SystemExit("--nbest needs --slots: the hypotheses are rows of the decoder pool")
    if args.nbest < 0:
        raise SystemExit("--nbest must be >= 0")
    if args.beams is not None:
        if not args.slots:
            raise SystemExit("--beams needs --slots: the beams are rows of the decoder pool")
        try:
            k = check_beam_args(args.beams, args.nbest or 1, 1.0 if args.length_penalty is None else args.length_penalty,
                                beam_early_stopping(args.early_stopping))[0]
        except ValueError as e:
            raise SystemExit(f"--beams / --nbest / --length-penalty / --early-stopping: {e}")
        if args.slots < k:
            raise SystemExit(f"--slots {args.slots} is below --beams {k}: an utterance's beams are rows of one pool")
    elif args.nbest:
        try:
            args.seed = int(check_sample_args(args.nbest, args.temperature, args.top_k, args.top_p, args.seed)[1].seed)
        except ValueError as e:
            raise SystemExit(f"--nbest / --temperature / --top-k / --top-p / --seed: {e}")


def beam_early_stopping(flag):
    """--early-stopping false | true | never (None = false) as ``beam_search_many`` takes it."""
    return {None: False, "false": False, "true": True, "never": "never"}[flag]


def check_long_args(args, ap):
    """``--long``: refuses the flags that do not go with it and bad segmentation parameters, resolves ``--slots`` (64) and, with
    ``--channels split``, ``--crosstalk-db`` (15); returns the segmentation parameters (segment.resolve_params)."""
    for flag, given in (("--split", bool(args.split)), ("--synthetic", args.synthetic > 0), ("--nbest", args.nbest != 0),
                        ("--batch-size", args.batch_size != ap.get_default("batch_size"))):
        if given:
            raise SystemExit(f"--long does not go with {flag}: every segment of a recording is a batch of one, decoded greedily")
    if args.ref is not None or args.ref_ids is not None:
        raise SystemExit("--long does not go with --ref / --ref-ids: score_errors --long compares a recording's joined segments with its reference")
    if not args.files:
        raise SystemExit("--long needs audio FILES")
    args.slots = args.slots or 64
    if not 1 <= args.slots <= 64 or args.pack < 1:
        raise SystemExit("--slots must be 1 .. 64 and --pack >= 1")
    given = {k: v for k, v in (("max_segment_s", args.max_segment_s), ("min_silence_s", args.min_silence_s), ("margin_db", args.vad_margin_db))
             if v is not None}
    try:
        vad = resolve_params(None, trim=not args.no_trim, **given)
    except ValueError as e:
        raise SystemExit(f"--max-segment-s / --min-silence-s / --vad-margin-db: {e}")
    if args.channels != "split":
        for flag, v in (("--crosstalk-db", args.crosstalk_db), ("--kaldi-text", args.kaldi_text)):
            if v is not None:
                raise SystemExit(f"{flag} needs --channels split: only there does a segment have a channel")
    else:
        args.crosstalk_db = 15.0 if args.crosstalk_db is None else args.crosstalk_db
        if not args.crosstalk_db >= 0.0:
            raise SystemExit(f"--crosstalk-db: crosstalk_db = {args.crosstalk_db:g} is NaN or negative (inf switches the gate off)")
    return vad


def load_long_tokenizer(args):
    """``--long``'s tokenizer (None: no "text"); ``--kaldi-text`` without one on disk is refused: its lines are text."""
    tok = load_tokenizer(args.tokenizer)
    if args.kaldi_text and tok is None:
        raise SystemExit("--kaldi-text needs a tokenizer found on disk (--tokenizer: an spm_char.model file or a directory holding one): its lines are text")
    return tok


# ---- decoding: both paths yield reference batches of Lines in corpus order ----------------------------------------------------------
@dataclass
class Run:
    """What the stages of one command share."""
    args: argparse.Namespace
    tok: Any
    scorer: Optional[RefScorer]
    model: Any
    processor: Any
    device: Any
    ngram: Any = None  # --ngram: the model, read once (load_ngram)


def span_sums(spans):
    """``math.fsum`` of every tensor of ``spans`` (1-D device tensors) after ONE read-back of them all."""
    flat = torch.cat(spans).cpu().tolist()
    ends = np.cumsum([t.shape[0] for t in spans]).tolist()
    return [math.fsum(flat[a:b]) for a, b in zip([0] + ends[:-1], ends)]


def line_errors(run, uids, rows):
    """Per row its "errors" (None without a reference, or without --ref / --ref-ids): one device pass for all of ``rows``."""
    if run.scorer is None:
        return [None] * len(rows)
    texts = [run.tok.decode(strip_special(r)) for r in rows] if run.tok is not None else None
    return run.scorer.errors(uids, rows, texts)


def batches_of(lines, size):
    """A window's Lines regrouped into the reference batches they were loaded as: ``size`` at a time, the last one what is left."""
    return [lines[k:k + size] for k in range(0, len(lines), size)]


def pair_lines(run, items):
    """Without --slots: encoder + ``generate`` per reference batch (then ``align``, then the references' pass), one batch of Lines each."""
    args, model = run.args, run.model
    for b0 in range(0, len(items), args.batch_size):
        chunk = items[b0:b0 + args.batch_size]
        f = load_batch(chunk, b0, run.processor, run.device)
        x, m = f["input_values"].to(run.device), f["attention_mask"].to(run.device)
        if args.scores:
            out = model.generate(x, m, max_length=args.max_length, return_dict_in_generate=True, output_scores=True)
            generated = (model._decoder_runtime.last_lengths - 1).tolist()
            rows, scores = out.sequences.cpu().tolist(), list(zip(out.sequence_logprobs.cpu().tolist(), generated))
        else:
            rows, scores = model.generate(x, m, max_length=args.max_length).cpu().tolist(), [None] * len(chunk)
        times = [None] * len(chunk)
        if args.timestamps:
            al = model.align(x, m, labels=timestamp_labels(rows))
            times = [token_times(al, i, row_length(r) - 1) for i, r in enumerate(rows)]
        uids = [uid for uid, _, _ in chunk]
        errs = line_errors(run, uids, rows)
        yield [Line(uid, r[:row_length(r)], s, t, None, e) for uid, r, s, t, e in zip(uids, rows, scores, times, errs)]


def greedy_window(run, feats):
    """(rows, their log-probability sums or None) of one window's batches through ``generate_many``."""
    args = run.args
    out = run.model.generate_many(feats, max_length=args.max_length, slots=args.slots, pack=args.pack, return_scores=args.scores)
    if not args.scores:
        return out, None
    rows, per_token = out
    return rows, span_sums(per_token)  # one read-back per window


def sampled_window(run, feats, first_utterance):
    """--nbest: (rows, their log-probability sums, per utterance its "nbest") of one window's batches through ``sample_many``.  The row
    is hypothesis 0 or, with --select mbr, the one of least risk (ties to the lowest index); every hypothesis is scored, so the row's
    sum is one of the sums the list was sorted by."""
    args = run.args
    hyps, hyp_scores = run.model.sample_many(feats, num_return_sequences=args.nbest, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                                             seed=args.seed, greedy_first=args.greedy_first, max_length=args.max_length, slots=args.slots,
                                             pack=args.pack, return_scores=True, first_utterance=first_utterance)
    sums = batches_of(span_sums([t for per in hyp_scores for t in per]), args.nbest)  # one read-back per window
    pick, risks = [0] * len(hyps), [None] * len(hyps)
    if args.select == "mbr":
        sel = metrics.mbr_select(hyps)
        pick = sel.best.cpu().tolist()
        risks = [r.cpu().tolist() for r in sel.risk]
    lists = [nbest_records(per, mine, run.tok, risk) for per, mine, risk in zip(hyps, sums, risks)]
    return [per[b] for per, b in zip(hyps, pick)], [mine[b] for mine, b in zip(sums, pick)], lists


def beam_window(run, feats):
    """--beams: (rows, their log-probability sums, per utterance its "nbest" or None) of one window's batches through
    ``beam_search_many``.  The row is the best beam or, with --select mbr, the one of least risk within the --nbest list.  With --ngram
    the sums are the fused ones and a fourth value, the rows' n-gram log-probabilities, follows (None without)."""
    args = run.args
    fusion = {}
    if args.ngram is not None:
        fusion = dict(lm=load_ngram(run), lm_weight=1.0 if args.lm_weight is None else args.lm_weight, lm_bonus=args.lm_bonus or 0.0)
    hyps = run.model.beam_search_many(feats, num_beams=args.beams, num_return_sequences=args.nbest or 1,
                                      length_penalty=1.0 if args.length_penalty is None else args.length_penalty,
                                      early_stopping=beam_early_stopping(args.early_stopping), max_length=args.max_length, slots=args.slots,
                                      pack=args.pack, **fusion)
    sums, scores = [t.tolist() for t in hyps.sequence_logprobs], [t.tolist() for t in hyps.sequence_scores]
    lm_sums = [t.tolist() for t in hyps.lm_logprobs] if fusion and args.scores else [None] * len(hyps)
    pick, risks = [0] * len(hyps), [None] * len(hyps)
    if args.select == "mbr":
        sel = metrics.mbr_select(hyps)
        pick = sel.best.cpu().tolist()
        risks = [r.cpu().tolist() for r in sel.risk]
    lists = [nbest_records(per, mine, run.tok, risk, sc, lm) for per, mine, risk, sc, lm in zip(hyps, sums, risks, scores, lm_sums)] if args.nbest else None
    return [per[b] for per, b in zip(hyps, pick)], [mine[b] for mine, b in zip(sums, pick)], lists, [lm and lm[b] for lm, b in zip(lm_sums, pick)]


def load_ngram(run):
    """--ngram: the ARPA file over the decoder's ids, read once per run; SystemExit naming the flag and what the file lacks."""
    if run.ngram is None:
        from .ngram import NgramLM
        vocab = run.model.speecht5.encoder._decoder_vocab
        try:
            run.ngram = NgramLM.from_arpa(run.args.ngram, vocab)
        except (OSError, ValueError) as e:
            raise SystemExit(f"--ngram {run.args.ngram}: not an ARPA model over the decoder's {vocab} ids: {e}")
    return run.ngram


def window_lines(run, items, starts):
    """The Lines of the batches that begin at ``starts``, loaded, encoded and decoded in the pool as one window."""
    args = run.args
    chunks = [items[b0:b0 + args.batch_size] for b0 in starts]
    feats = [load_batch(chunk, b0, run.processor, run.device) for chunk, b0 in zip(chunks, starts)]
    lists = lm_sums = None
    if args.beams is not None:
        rows, sums, lists, lm_sums = beam_window(run, feats)
    elif args.nbest:
        rows, sums, lists = sampled_window(run, feats, starts[0])
    else:
        rows, sums = greedy_window(run, feats)
    ids, n = [r.tolist() for r in rows], len(rows)
    scores = [(v, len(r) - 1) for v, r in zip(sums, ids)] if args.scores else [None] * n
    stamps = [None] * n
    if args.timestamps:  # the utterances' own tokens after the start token: no padding inside align_many's input
        als = run.model.align_many(feats, [r[1:] for r in rows], pack=args.pack)
        stamps = [rounded_pairs(zip(al.start_times.cpu().tolist(), al.end_times.cpu().tolist())) for al in als]
    uids = [uid for chunk in chunks for uid, _, _ in chunk]
    errs = line_errors(run, uids, ids)  # one pass per window
    return [Line(*fields) for fields in zip(uids, ids, scores, stamps, lists or [None] * n, errs, lm_sums or [None] * n)]


def pool_lines(run, items):
    """With --slots: ``max(--pack, 4 * --slots)`` batches per window, each window's Lines handed on a reference batch at a time."""
    args = run.args
    starts = list(range(0, len(items), args.batch_size))
    window = max(args.pack, 4 * args.slots)
    for w0 in range(0, len(starts), window):
        yield from batches_of(window_lines(run, items, starts[w0:w0 + window]), args.batch_size)


def transcribe_recording(run, path, vad):
    """The LongTranscript of one file: ``transcribe_channels`` on its channels with --channels split, ``transcribe_long`` on their mean."""
    args, split = run.args, run.args.channels == "split"
    x = (load_audio_channels_16k if split else load_audio_16k)(path, device=run.device)
    x = (x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, dtype=np.float32))).to(run.device)
    common = dict(vad=vad, max_length=args.max_length, slots=args.slots, pack=args.pack, return_scores=args.scores, timestamps=args.timestamps,
                  do_normalize=args.do_normalize)
    return run.model.transcribe_channels(x, crosstalk_db=args.crosstalk_db, **common) if split else run.model.transcribe_long(x, **common)


def main_long(args, ap):
    """``--long``: every FILE is one recording; with ``--channels split`` every channel of it is cut and decoded on its own."""
    vad = check_long_args(args, ap)
    tok = load_long_tokenizer(args)
    model = build_model(args)
    run = Run(args, tok, None, model, None, torch.device("cuda", torch.cuda.current_device()))
    with open_outputs(args) as (fh, kh):
        for path in args.files:
            write_recording(fh, kh, path, transcribe_recording(run, path, vad), run)
    return 0


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m loco-asr_amd.transcribe", description=__doc__.split("\n\n")[0])
    ap.add_argument("--pretrained", default=None, metavar="DIR", help="HuggingFace SpeechT5ForSpeechToText checkpoint on disk (never downloaded)")
    ap.add_argument("--random-init", action="store_true", help="deterministic synthetic weights (no checkpoint available)")
    ap.add_argument("files", nargs="*", metavar="FILE", help="audio files (.wav / .flac) to transcribe, in this order")
    ap.add_argument("--data-path", default="slurp", help="SLURP root (dataset/slurp/<split>.jsonl, audio/slurp_real), as extract.py")
    ap.add_argument("--split", "-s", choices=["train", "devel", "test", "train_synthetic"], default=None)
    ap.add_argument("--do-normalize", action="store_true", help="zero-mean unit-variance waveforms, as the HF feature extractor's do_normalize")
    ap.add_argument("--synthetic", type=int, default=0, help="transcribe N seeded synthetic clips")
    ap.add_argument("--synthetic-seconds", type=float, default=5.0)
    ap.add_argument("--batch-size", type=int, default=2, help="utterances per generate call (the reference's loop: 2)")
    ap.add_argument("--max-length", type=int, default=100, help="total tokens per utterance, start token included (the reference's notebooks: 100)")
    ap.add_argument("--slots", type=int, default=0, help="decode in a pool of N rows with finished rows refilled (1 .. 64); 0 = one generate call per batch")
    ap.add_argument("--pack", type=int, default=8, metavar="G", help="with --slots: batches per packed encoder forward")
    ap.add_argument("--nbest", type=int, default=0, metavar="N", help="with --slots: also write \"nbest\", N sampled transcripts sorted by logprob (1 .. 64); the "
                    "line's other fields are then hypothesis 0, which is the greedy transcript ONLY with --greedy-first and a sampled one otherwise")
    ap.add_argument("--temperature", type=float, default=1.0, help="with --nbest: logits are divided by it before the draw")
    ap.add_argument("--top-k", type=int, default=0, help="with --nbest: draw among the k most likely tokens (0 = off)")
    ap.add_argument("--top-p", type=float, default=1.0, help="with --nbest: draw within the smallest set of tokens of probability mass >= p (1 = off)")
    ap.add_argument("--seed", type=int, default=None, help="with --nbest: the random numbers' seed (default: drawn from torch's generator)")
    ap.add_argument("--greedy-first", action="store_true", help="with --nbest: hypothesis 0 is the greedy transcript, so the line's own fields are what they "
                    "are without --nbest")
    ap.add_argument("--beams", type=int, default=None, metavar="K", help="with --slots >= K: beam search with K beams (1 .. 16) instead of greedy search; "
                    "--nbest N (N <= K) then lists the N best beams with their \"score\"")
    ap.add_argument("--length-penalty", type=float, default=None, help="with --beams: a hypothesis scores its log-probability over length ** this (default 1)")
    ap.add_argument("--early-stopping", choices=["false", "true", "never"], default=None, help="with --beams: HF's early_stopping (default false)")
    ap.add_argument("--ngram", default=None, metavar="ARPA", help="with --beams: shallow fusion of a character n-gram model over the decoder's ids "
                    "(python -m loco-asr_amd.ngram trains one); \"logprob\" and \"score\" are then the fused values and --scores adds \"lm_logprob\"")
    ap.add_argument("--lm-weight", type=float, default=None, help="with --ngram: the weight of the model's log-probability (default 1)")
    ap.add_argument("--lm-bonus", type=float, default=None, help="with --ngram: added per generated token (default 0)")
    ap.add_argument("--scores", action="store_true", help="also write \"logprob\" (sum over the generated tokens) and \"avg_logprob\" (per generated token)")
    ap.add_argument("--timestamps", action="store_true", help="also write \"token_times\": [start_s, end_s] of every generated token (cross-attention + DTW)")
    ap.add_argument("--tokenizer", default=None, help="spm_char.model file or a directory holding one; found on disk -> \"text\" is written too")
    ap.add_argument("--precision", choices=["f16x3", "f32", "f16x2"], default="f16x3", help="arithmetic of the ENCODER (the decoder is fp32)")
    ap.add_argument("--out", default="-", help="JSON-lines file, - = stdout")
    ap.add_argument("--long", action="store_true", help="FILES are whole recordings: cut each at pauses on the device, one JSON line per recording")
    ap.add_argument("--max-segment-s", type=float, default=None, help="with --long: longest segment in seconds (default 20)")
    ap.add_argument("--min-silence-s", type=float, default=None, help="with --long: shortest pause that counts as one (default 0.3)")
    ap.add_argument("--vad-margin-db", type=float, default=None, help="with --long: speech is this far above the noise level (default 10)")
    ap.add_argument("--no-trim", action="store_true", help="with --long: keep each segment's leading and trailing silence (segments then tile the recording)")
    ap.add_argument("--channels", choices=["mix", "split"], default=None, help="with --long: mix (default) averages a file's channels into one "
                    "recording; split cuts and decodes every channel on its own (one speaker per channel, as in a two-channel telephone call)")
    ap.add_argument("--crosstalk-db", type=float, default=None, help="with --channels split: a frame is not speech when another channel is louder "
                    "there by more than this (default 15; inf = no gate)")
    ap.add_argument("--kaldi-text", default=None, metavar="FILE", help="with --channels split and a tokenizer on disk: also write Kaldi 'utt_id text' "
                    "lines, <rec>-<A|B>-<start>-<end> in centiseconds, the input of eval_ppl")
    ap.add_argument("--select", choices=["first", "mbr"], default=None, help="with --nbest: which hypothesis the line's own fields are: first "
                    "(default) = hypothesis 0, as ever; mbr = the one of least expected edit distance to the list's others (token ids, every "
                    "sample weighing 1), and every \"nbest\" entry also carries \"mbr_risk\"")
    ap.add_argument("--ref", nargs="?", const="", default=None, metavar="FILE", help="Kaldi 'utt_id text' references: every line with one also gets "
                    "\"errors\" (cer, wer and the character-level sub / del / ins / ref_len), the corpus %%CER / %%WER go to stderr; without FILE, "
                    "with --split, the SLURP sentences of the split.  Needs a tokenizer on disk (--tokenizer): the comparison is of text")
    ap.add_argument("--ref-ids", default=None, metavar="FILE", help="'utt_id id id ...' references: as --ref on token ids (<s>, </s>, <pad> dropped on "
                    "both sides), no tokenizer needed; \"errors\" then has no wer")
    return ap


def report(scorer):
    """The corpus %CER / %WER lines of --ref / --ref-ids, to stderr."""
    if scorer is not None:
        for line in scorer.report():
            print(line, file=sys.stderr)


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    check_args(args, ap)
    if args.long:
        return main_long(args, ap)
    items = gather_items(args)
    tok = load_tokenizer(args.tokenizer)
    scorer = load_references(args, tok)  # refused here, before a model is built
    processor = SpeechT5FeatureExtractorMI355X(do_normalize=args.do_normalize)
    model = build_model(args)
    run = Run(args, tok, scorer, model, processor, torch.device("cuda", torch.cuda.current_device()))
    with open_outputs(args) as (fh, _):
        for batch in (pool_lines if args.slots else pair_lines)(run, items):
            write_lines(fh, batch, tok)
    report(scorer)
    return 0


if __name__ == "__main__":
    sys.exit(main())
