"""Per-recording GPT-2 perplexity of a transcript file: ``python -m loco-asr_amd.eval_ppl``.

The flags of the reference's ``lms/src/eval_ppl_with_pretrained_lm.py`` (``--in_file``, ``--out_dir``, ``--bsize``, ``--context_type``,
``--model``) and its two output files, ``rec_id2nlls.pkl`` and ``rec_id2ppl.json``, plus the log line with the mean, standard deviation,
minimum and maximum perplexity.  Nothing is downloaded: ``--pretrained DIR`` names a checkpoint directory on disk, ``--random-init``
builds the synthetic weight family of ``synth.gpt2_state_dict``.  ``--tokenized`` reads ``utt_id id id ...`` lines; without it the
checkpoint directory must hold GPT-2's tokenizer files.

``--context_type carry`` is this project's third mode and not the reference's: a K/V cache is carried from utterance to utterance of a
recording and rebuilt from the last ``--keep`` tokens when it is full -- HuggingFace's strided perplexity with utterance-aligned strides.
Every token but a recording's first is scored once, behind ``--keep`` .. ``n_positions - 1`` tokens of context, where ``max_len`` gives
every token the full window at the price of one forward per token.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import pickle
import sys
import time

import numpy as np


class TokenizerFilesMissing(FileNotFoundError):
    """``--pretrained DIR`` holds no tokenizer files and ``--tokenized`` was not given."""


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="loco-asr_amd.eval_ppl", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--in_file", "-in_file", "-i", required=True, help="'utt_id text' lines; utt_id = rec-x-start-end, the recording is utt_id up to the first '-'")
    p.add_argument("--out_dir", "-o", required=True, help="where rec_id2nlls.pkl, rec_id2ppl.json and the log are written")
    p.add_argument("--bsize", "--batch_size", "-bsize", "-batch_size", "--sb", "-sb", type=int, default=128, help="max batch size")
    p.add_argument("--model", "-model", "-m", default="gpt2", choices=["gpt2"], help="only GPT-2 base (768 wide) is implemented")
    p.add_argument("--context_type", "-context_type", "--ct", "-ct", choices=["indep", "max_len", "carry"], default="indep",
                   help="indep: every utterance alone; max_len: the recording's left context up to n_positions tokens (the reference's stride-1 "
                        "windows); carry: a K/V cache carried from utterance to utterance, HuggingFace's strided perplexity with utterance-aligned "
                        "strides -- NOT the reference's max_len: a token sees between --keep and n_positions - 1 tokens of context")
    p.add_argument("--keep", type=int, default=None, help="carry: tokens of context kept when the cache is rebuilt (default n_positions // 2)")
    p.add_argument("--inflight", type=int, default=8, help="carry: recordings walked in lock-step, one cache slot each (1 .. 64)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--pretrained", metavar="DIR", help="HuggingFace GPT-2 checkpoint directory on disk (config.json + model.safetensors / pytorch_model.bin)")
    src.add_argument("--random-init", action="store_true", help="synthetic weights (synth.gpt2_state_dict) with --layers / --positions / --vocab")
    p.add_argument("--layers", type=int, default=12)
    p.add_argument("--positions", type=int, default=1024)
    p.add_argument("--vocab", type=int, default=50257)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--tokenized", action="store_true", help="input lines are 'utt_id id id ...'")
    p.add_argument("--no-strict-reference", dest="strict_reference", action="store_false",
                   help="max_len: also score a recording's final token and recordings of exactly n_positions tokens, which the reference skips")
    p.add_argument("--verbose", "-v", action="store_true")
    return p


def load_tokenizer(args, vocab):
    from . import lm
    if args.tokenized:
        return lm.TokenizedLines(eos_token_id=vocab - 1)
    d = args.pretrained
    if not d or not (os.path.exists(os.path.join(d, "tokenizer.json")) or
                     (os.path.exists(os.path.join(d, "vocab.json")) and os.path.exists(os.path.join(d, "merges.txt")))):
        raise TokenizerFilesMissing(f"{d or '--random-init'}: no tokenizer.json or vocab.json + merges.txt on disk; tokenize the corpus elsewhere and pass --tokenized")
    from transformers import GPT2TokenizerFast
    return GPT2TokenizerFast.from_pretrained(d, local_files_only=True)


def summary_line(rec_id2ppl) -> str:
    ppls = np.asarray(list(rec_id2ppl.values()), np.float64)
    return (f"Avg. PPL of recordings: {np.mean(ppls):.2f} std.dev: {np.std(ppls):.2f} min PPL: {np.min(ppls):.2f} "
            f"max PPL: {np.max(ppls):.2f}")


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    import torch
    from . import lm, synth
    if not torch.cuda.is_available():
        raise RuntimeError("eval_ppl needs a ROCm device: the language model has no CPU path")
    os.makedirs(args.out_dir, exist_ok=True)
    base = os.path.basename(args.in_file).rsplit(".", 1)[0]
    log_path = os.path.join(args.out_dir, f"{args.model}_{args.context_type}_{base}.log")
    logger = logging.getLogger("loco.eval_ppl")
    logger.setLevel(logging.INFO)
    logger.handlers = [logging.FileHandler(log_path)] + ([logging.StreamHandler()] if args.verbose else [])
    for h in logger.handlers:
        h.setFormatter(logging.Formatter("%(asctime)s %(message)s", "%d-%m-%Y %H:%M:%S"))

    if args.random_init:
        sd = synth.gpt2_state_dict(args.seed, args.layers, args.positions, args.vocab)
        model = lm.GPT2LMHeadModelMI355X.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    else:
        model = lm.GPT2LMHeadModelMI355X.from_pretrained(args.pretrained)
    model.to("cuda")
    tokenizer = load_tokenizer(args, model.vocab_size)
    utts = lm.read_key_text(args.in_file)
    t0 = time.time()
    if args.context_type == "indep":
        rec_id2nlls, rec_id2ppl = lm.score_indep(model, utts, tokenizer, args.bsize)
    elif args.context_type == "carry":
        rec_id2nlls, rec_id2ppl = lm.score_carry(model, utts, tokenizer, keep=args.keep, inflight=args.inflight)
    else:
        rec_id2nlls, rec_id2ppl = lm.score_max_len(model, utts, tokenizer, args.bsize, strict_reference=args.strict_reference)
    with open(os.path.join(args.out_dir, "rec_id2nlls.pkl"), "wb") as fh:
        pickle.dump(rec_id2nlls, fh)
    with open(os.path.join(args.out_dir, "rec_id2ppl.json"), "w", encoding="utf-8") as fh:
        json.dump(rec_id2ppl, fh, indent=2, ensure_ascii=False)
    if rec_id2ppl:
        logger.info(summary_line(rec_id2ppl))
    n_tok = sum(len(v) for v in rec_id2nlls.values())
    logger.info(f"Saved in {args.out_dir} Time taken {time.time() - t0:.2f} sec ({n_tok} tokens scored, {len(rec_id2ppl)} recordings)")
    for h in logger.handlers:
        h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
