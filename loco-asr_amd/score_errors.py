"""Error rates of transcripts against references: ``python -m loco-asr_amd.score_errors --ref text --hyp {text | out.jsonl}``.

``--ref`` is a Kaldi ``utt_id text`` file.  ``--hyp`` is another one, or this project's JSON lines (``transcribe``'s output: a line's
"id" and "text").  Utterances are matched by id; the ones present on one side only are counted and left out.  ``--unit word`` prints a
``%WER`` line, ``--unit char`` a ``%CER`` line, neither flag both, in the form of Kaldi's compute-wer:
``%WER 12.34 [ 123 / 997, 10 ins, 40 del, 73 sub ]``.  ``--per-utt FILE`` also writes one such line per utterance and unit.

``--long``: a recording is the unit.  The hypothesis is a ``transcribe --long`` line -- its segments' texts joined in time order -- or the
Kaldi lines ``transcribe --kaldi-text`` wrote, joined per recording; the reference's lines ``<rec>-...`` are joined per recording
likewise (by the start field of ``<rec>-<channel>-<start>-<end>`` where the ids have that form, in file order otherwise).

The distances are computed on the device (metrics.edit_counts, csrc/edit_distance.hip) under the project's rule -- minimum cost, then
most correct symbols: the error counts and rates are sclite's and Kaldi's, the split into ins / del / sub can differ from theirs
where alignments tie.  Text is compared as it stands (no case folding, no punctuation rules) with runs of whitespace as one blank.
Exit code 1 when no utterance matched.
"""
from __future__ import annotations

import argparse
import json
import re
import sys
from collections import OrderedDict

from .lm import read_key_text, rec_id_of

_TIMED_ID = re.compile(r"^(?P<rec>[^-]+)-(?P<ch>[^-]+)-(?P<start>\d+)-(?P<end>\d+)$")


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m loco-asr_amd.score_errors", description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", required=True, metavar="FILE", help="Kaldi 'utt_id text' references")
    ap.add_argument("--hyp", required=True, metavar="FILE", help="Kaldi 'utt_id text' hypotheses, or transcribe's JSON lines")
    ap.add_argument("--unit", choices=["word", "char"], default=None, help="what is compared (default: both, a %%WER and a %%CER line)")
    ap.add_argument("--per-utt", default=None, metavar="FILE", help="also write one line per utterance and unit: 'utt_id %%WER ...'")
    ap.add_argument("--long", action="store_true", help="compare whole recordings: segments (hypothesis) and utterance lines (reference) are "
                    "joined per recording in time order")
    return ap


def rec_key(name: str) -> str:
    """A recording's id from its name: ``-`` and whitespace as ``_``, so that ``rec_id_of`` (an utterance id up to its first ``-``) finds
    it again.  THE definition: transcribe's --kaldi-text ids (``kaldi_rec_id``) and --long's JSON ids here go through it."""
    return "".join("_" if ch == "-" or ch.isspace() else ch for ch in name)


def join_recordings(utts) -> "OrderedDict[str, str]":
    """Kaldi lines -> {recording: its lines' texts joined}: by the ids' start field when every line of the recording has the form
    ``<rec>-<channel>-<start>-<end>`` (ties by channel, then file order), in file order otherwise.  A pure function."""
    groups: "OrderedDict[str, list]" = OrderedDict()
    for n, (uid, text) in enumerate(utts.items()):
        m = _TIMED_ID.match(uid)
        groups.setdefault(rec_id_of(uid), []).append(((int(m.group("start")), m.group("ch")) if m else None, n, text))
    out = OrderedDict()
    for rec, rows in groups.items():
        if all(key is not None for key, _, _ in rows):
            rows = sorted(rows, key=lambda r: (r[0], r[1]))
        out[rec] = " ".join(text for _, _, text in rows)
    return out


def read_hyp(path: str, long_form: bool) -> "OrderedDict[str, str]":
    """{id: text} of a hypothesis file: JSON lines when the first non-blank character is ``{``, Kaldi text otherwise."""
    with open(path, "r", encoding="utf-8") as fh:
        head = fh.read(4096).lstrip()
    if not head.startswith("{"):
        utts = read_key_text(path)
        return join_recordings(utts) if long_form else utts
    out: "OrderedDict[str, str]" = OrderedDict()
    with open(path, "r", encoding="utf-8") as fh:
        for n, line in enumerate(fh, 1):
            if not line.strip():
                continue
            rec = json.loads(line)
            if long_form:
                if "segments" not in rec:
                    raise SystemExit(f"{path}:{n}: --long expects transcribe --long lines (no \"segments\")")
                segs = sorted(enumerate(rec["segments"]), key=lambda s: (s[1]["start_s"], s[0]))
                if any("text" not in s for _, s in segs):
                    raise SystemExit(f"{path}:{n}: a segment has no \"text\" (transcribe needs --tokenizer on disk to write it)")
                out.setdefault(rec_key(str(rec["id"])), " ".join(s["text"] for _, s in segs))
            else:
                if "text" not in rec:
                    raise SystemExit(f"{path}:{n}: the line has no \"text\" (transcribe needs --tokenizer on disk to write it; "
                                     "transcribe --ref-ids compares token ids)")
                out.setdefault(str(rec["id"]), rec["text"])
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    refs = read_key_text(args.ref)
    if args.long:
        refs = join_recordings(refs)
    hyps = read_hyp(args.hyp, args.long)
    ids = [u for u in refs if u in hyps]
    only_ref, only_hyp = len(refs) - len(ids), len(hyps) - len(ids)
    what = "recordings" if args.long else "utterances"
    if not ids:
        print(f"no {what} matched: {only_ref} only in --ref, {only_hyp} only in --hyp", file=sys.stderr)
        return 1
    from . import metrics
    per = open(args.per_utt, "w", encoding="utf-8") if args.per_utt else None
    try:
        for unit, name in (("word", "WER"), ("char", "CER")):
            if args.unit not in (None, unit):
                continue
            table = metrics.count_table([refs[u] for u in ids], [hyps[u] for u in ids], unit)
            print(metrics.format_kaldi_line(name, *(sum(row) for row in table)))
            if per is not None:
                for n, u in enumerate(ids):
                    per.write(f"{u} {metrics.format_kaldi_line(name, *(row[n] for row in table))}\n")
    finally:
        if per is not None:
            per.close()
    print(f"scored {len(ids)} {what}; {only_ref} only in --ref, {only_hyp} only in --hyp")
    return 0


if __name__ == "__main__":
    sys.exit(main())
