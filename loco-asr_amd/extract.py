#!/usr/bin/env python3
"""Drop-in for the audio branch of the reference's extraction scripts
(/root/reference/speech_text/extract_speecht5_base_embeddings_slurp.py:96-113 and
extract_speecht5_finetuned_embeddings_slurp.py:93-113) on MI355X.

    python loco-asr_amd/extract.py -m audio -s train                       # SLURP layout under ./slurp
    python loco-asr_amd/extract.py -m audio -s devel --synthetic 64        # no corpus: seeded synthetic clips
    torchrun --standalone --nproc-per-node 8 loco-asr_amd/extract.py -m audio -s train     # data parallel

Same flags (-m/--modality, -s/--split), same folder layout (extracted/<model>/<split>/<modality>/), the same
per-utterance pickle and THE SAME BATCHES as the reference: ``batch_size = 2``, ``shuffle=False``, corpus order
(…base…py:67-68).  Batch composition is part of the function -- GroupNorm statistics run over the padded axis, so an
utterance encoded next to a longer one differs from the same utterance encoded alone -- and the
reference's pairs (0,1), (2,3), ... are therefore kept at every world size: with WORLD_SIZE > 1 whole batches are dealt
round-robin to the ranks (dp.shard_batches); each rank writes the files of its own batches, so no embedding crosses the
fabric unless --gather is given.  ``--batch-size N`` / ``--bucket-by-length`` trade that identity for throughput
(bigger batches; units sorted by length so that padding is minimal) and say so in their help text.

What differs by necessity: weights come from ``--prenet-state-dict`` / ``--encoder-state-dict`` /
``--text-prenet-state-dict`` (the pickled dicts the base script loads from extracted/speecht5/mapping/, …base…py:40-49)
or ``--random-init``, or from a checkpoint directory on disk (``--pretrained DIR``: the fine-tuned script's ``from_pretrained``
without the hub download); audio decoding needs no libsndfile -- 16 / 32-bit PCM and float WAV files and FLAC files (SLURP's format)
are decoded by audio_io.py (read_pcm_wav; the library's loco_flac_decode, CRC- and MD5-verified), anything else through soundfile when
it is installed -- followed by the device polyphase resampler to 16 kHz; ``-m text`` (…base…py:79-93) needs the tokenizer files in a
local directory.  Targets are one-hot over the reference's fixed 101 intent labels (``ALL_CLASSES``, …base…py:32-36),
shipped as loco-asr_amd/data/slurp_intent_classes.txt, for every split alike.

main() is a sequence of stages: parse_args, setup_rank, load_units, load_model, plan_batches, then one ordered producer / consumer
loop (run_ordered) between ``forwards`` -- Staging's batches or packs, each enqueued on the GPU -- and a ``Finisher``, then report.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import pickle
import queue
import sys
import threading
import time
import traceback
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
la = importlib.import_module("loco-asr_amd")
dp = importlib.import_module("loco-asr_amd.dp")
sink_mod = importlib.import_module("loco-asr_amd.sink")
audio_io = importlib.import_module("loco-asr_amd.audio_io")


def read_slurp_split(data_path: str, split: str):
    """(slurp_id, sentence, wav_path, 16000, intent) per utterance, the tuple contract of the reference's
    SLURPDataset (slurp_data.py:19-66): headset recording if there is one, else the first."""
    text_path = os.path.join(data_path, "dataset/slurp", split + ".jsonl")
    audio_dir = os.path.join(data_path, "audio", "slurp_synth" if split == "train_synthetic" else "slurp_real")
    items = []
    with open(text_path) as fh:
        for line in fh:
            if not line.strip():
                continue
            item = json.loads(line)
            rec = next((r["file"] for r in item["recordings"] if "headset" in r), item["recordings"][0]["file"])
            items.append((item["slurp_id"], item["sentence"], os.path.join(audio_dir, rec), 16000, item["intent"]))
    return items


CLASSES_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "slurp_intent_classes.txt")


def load_classes(path=None):
    """The reference's ALL_CLASSES (intent_classes.py, used at …base…py:32): the fixed 101 SLURP intent labels, the same for
    every split -- never the labels that happen to occur in the split being extracted (train has 91 of them, train_synthetic
    98: targets of different widths and index maps would result)."""
    with open(path or CLASSES_FILE) as fh:
        classes = [l.strip() for l in fh if l.strip()]
    if len(classes) != 101 or len(set(classes)) != 101:
        raise SystemExit(f"{path or CLASSES_FILE}: expected 101 distinct intent labels, found {len(classes)} "
                         f"({len(set(classes))} distinct): IntentClassifier's output layer is Linear(768, 101)")
    return classes


def one_hot_encoder(classes):
    """LabelEncoder + LabelBinarizer of the reference (…base…py:32-36): classes sorted, one-hot int64 rows."""
    order = sorted(set(classes))
    index = {c: i for i, c in enumerate(order)}
    eye = np.eye(len(order), dtype=np.int64)

    def encode(labels):
        unknown = [l for l in labels if l not in index]
        if unknown:  # sklearn's LabelEncoder.transform raises ValueError("y contains previously unseen labels") here
            raise ValueError(f"y contains previously unseen labels: {unknown}")
        return np.stack([eye[index[l]] for l in labels])
    return encode


def load_state_dict_file(path):
    with open(path, "rb") as fh:
        sd = pickle.load(fh)
    return {k: (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))) for k, v in sd.items()}


def load_model(args, device, text=False):
    """The speech model (or, ``text``, the text model) on ``device`` from one of the three weight sources: the pickled state dicts,
    --random-init's deterministic synthetic weights, or (speech only) a --pretrained checkpoint on disk."""
    if args.pretrained:
        model = la.SpeechT5ForSpeechToTextMI355X.from_pretrained(args.pretrained)
    else:
        if args.random_init:
            pre, enc_sd = la.synth.split_state_dict(la.synth.encoder_state_dict(0))
            if text:
                pre = {k[len("text_prenet."):]: v for k, v in la.synth.text_prenet_state_dict(0).items()}
            pre = {k: torch.from_numpy(np.asarray(v)) for k, v in pre.items()}
            enc_sd = {k: torch.from_numpy(v) for k, v in enc_sd.items()}
        else:
            pre = load_state_dict_file(args.text_prenet_state_dict if text else args.prenet_state_dict)
            enc_sd = load_state_dict_file(args.encoder_state_dict)
        model = (la.SpeechT5ForTextToSpeechMI355X if text else la.SpeechT5ForSpeechToTextMI355X).from_state_dicts(pre, enc_sd)
    model = model.to(device)
    print("Loaded model")
    model.eval()
    return model


def run_ordered(work, finish, depth, threaded=False, name=None, init=None):
    """``finish(item)`` for every item of the iterator ``work``, once each and in the order ``work`` produces them, with up to
    ``depth`` items between the two.  Returns the failures, first one first; an empty list when there was none.

    Unthreaded: items wait in a deque and the oldest is finished while ``depth`` are pending (``depth`` 1: finished at once).
    Threaded: two host threads share the loop -- this one runs ``work``, a consumer thread called ``name`` runs ``init()`` and
    then finishes each item IN ORDER.  The queue between them is bounded: at most ``depth`` items wait behind the one being
    finished.  A failure on the consumer is recorded, and the consumer keeps draining so that the producer never blocks on a dead
    consumer; the producer stops at the next item.  A failure of ``work`` itself is put first, and what it produced before is
    still finished.  The consumer is always joined."""
    failures = []
    if not threaded:
        pending, work = deque(), iter(work)

        def finish_down_to(n):
            try:
                while len(pending) > n:
                    finish(pending.popleft())
            except BaseException as e:  # noqa: BLE001 -- the caller decides; what is still pending is dropped, as the consumer thread does
                failures.append(e)
                pending.clear()

        while not failures:
            try:
                pending.append(next(work))
            except StopIteration:
                break
            except BaseException as e:  # noqa: BLE001 -- what was produced before it is still finished, as the consumer thread does
                failures.append(e)
                break
            finish_down_to(depth - 1)
        finish_down_to(0)
        return failures
    todo = queue.Queue(maxsize=depth)

    def consume():
        try:
            if init is not None:
                init()
            while True:
                item = todo.get()
                if item is None:
                    return
                finish(item)
        except BaseException as e:  # noqa: BLE001 -- handed to the producing thread
            failures.append(e)
            while todo.get() is not None:  # keep draining so that the producer never blocks on a dead consumer
                pass

    consumer = threading.Thread(target=consume, name=name)
    consumer.start()
    try:
        for item in work:
            todo.put(item)
            if failures:
                break
    except BaseException as e:  # noqa: BLE001 -- a failure of THIS thread (an unreadable file, a refused forward): reported like the consumer's
        failures.insert(0, e)
    finally:
        todo.put(None)
        consumer.join()
    return failures


def padded_ids(seqs):
    T = max(len(q) for q in seqs)
    ids = np.full((len(seqs), T), 1, dtype=np.int64)  # padding="longest" with pad_token_id = 1
    for r, q in enumerate(seqs):
        ids[r, :len(q)] = q
    return torch.from_numpy(ids)


def text_forwards(enc, batches, tokenize, device, inflight, pack):
    """(unit indices, BaseModelOutput or ticket) per batch of transcripts; with --pack G (the index lists of G batches, the ticket
    of their one forward): every row's keys end where its own batch ends (text_encoder.forward_packed)."""
    if pack:
        for g0 in range(0, len(batches), pack):
            group = batches[g0:g0 + pack]
            yield group, enc.forward_packed_async([padded_ids(tokenize(idx)) for idx in group])
    else:
        for idx in batches:
            dev_ids = padded_ids(tokenize(idx)).to(device)
            yield idx, (enc.forward_async(dev_ids) if inflight > 1 else enc(dev_ids))


def extract_text(args, items, encode_labels, device, world, rank):
    """The reference's text branch (…base…py:79-93): SpeechT5ForTextToSpeech(...).speecht5.encoder(texts.input_ids) -- ids
    padded to the longest transcript of the batch with <pad> = 1 and NO attention mask -- one pickle per utterance."""
    model = load_model(args, device, text=True)
    if args.synthetic:
        lens = [8 + (37 * i) % 90 for i in range(len(items))]
        tokenize = lambda idx: [la.synth.token_ids(1, lens[i], seed=100 + i)[0][0] for i in idx]
    else:
        try:
            from transformers import SpeechT5Tokenizer
            tok = SpeechT5Tokenizer.from_pretrained(args.tokenizer)
        except Exception as e:  # no hub access / no local files: say what is needed instead of a stack trace
            raise SystemExit(f"-m text needs the SpeechT5 tokenizer files (--tokenizer DIR with spm_char.model): {e}")
        tokenize = lambda idx: [np.asarray(tok(items[i][1])["input_ids"], dtype=np.int64) for i in idx]
    enc = model.speecht5.encoder
    enc.precision, enc.range_policy = getattr(args, "precision", enc.precision), getattr(args, "range_policy", enc.range_policy)
    inflight = args.inflight if args.inflight > 0 else 4
    pack = max(0, getattr(args, "pack", 0))
    if inflight > 1 or pack:
        enc.set_inflight(inflight)  # batches of transcripts are tiny (<= 2 x ~100 tokens): several in flight, results untouched
    my = dp.shard_batches(len(items), args.batch_size, world, rank)  # the reference's batches, dealt whole
    with torch.no_grad(), sink_mod.EmbeddingSink(args.out, args.split, args.modality, args.format) as sink:
        def finish(item):
            meta, res = item
            res = res.result() if hasattr(res, "result") else res
            # --pack: meta = the index lists of the pack's batches, res = one output per batch
            for idx, o in zip(meta, res) if pack else [(meta, res)]:
                sink.submit([items[i][0] for i in idx], o.last_hidden_state, encode_labels([items[i][4] for i in idx]))

        failures = run_ordered(text_forwards(enc, my, tokenize, device, inflight, pack), finish, inflight)
        if failures:
            raise failures[0]
    print("Done!")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Extract SpeechT5 speech-encoder embeddings on MI355X")
    ap.add_argument("--modality", "-m", choices=["text", "audio"], required=True)
    ap.add_argument("--split", "-s", choices=["train", "devel", "test", "train_synthetic"], required=True)
    ap.add_argument("--data-path", default="slurp")
    ap.add_argument("--out", default=None,
                    help="output root; default extracted/speecht5_base (the base script's, …base…py:70) or, with --pretrained, "
                         "extracted/speecht5 (the fine-tuned script's, …finetuned…py:63-64)")
    ap.add_argument("--pretrained", default=None, metavar="DIR",
                    help="the fine-tuned script's weights (…finetuned…py:95: SpeechT5ForSpeechToText.from_pretrained('microsoft/speecht5_asr')) "
                         "from a checkpoint ON DISK: a directory with model.safetensors / pytorch_model.bin, such a file, or a hub name "
                         "already in the local HuggingFace cache (never downloaded); replaces the two --*-state-dict pickles")
    ap.add_argument("--resume", action="store_true",
                    help="skip every reference batch whose utterances all have their output file already (whole batches only: batch "
                         "composition is part of the function, a batch is never re-formed around a missing member)")
    ap.add_argument("--batch-size", type=int, default=2,
                    help="default 2 = the reference's batch_size (…base…py:67); batch composition changes the embeddings of padded "
                         "utterances (GroupNorm over the padded axis), so other values are not bit-comparable with the reference")
    ap.add_argument("--bucket-by-length", action="store_true",
                    help="sort units by length and deal them to ranks longest first (minimal padding, balanced T^2 work) instead of "
                         "the reference's corpus-order batches; changes which utterances share a batch")
    ap.add_argument("--prenet-state-dict", default="extracted/speecht5/mapping/speech_prenet_state_dict.pickle")
    ap.add_argument("--encoder-state-dict", default="extracted/speecht5/mapping/encoder_state_dict.pickle")
    ap.add_argument("--random-init", action="store_true", help="deterministic synthetic weights (no checkpoint available)")
    ap.add_argument("--synthetic", type=int, default=0, help="encode N seeded synthetic clips instead of a corpus")
    ap.add_argument("--synthetic-seconds", type=float, default=5.0)
    ap.add_argument("--synthetic-min-seconds", type=float, default=None,
                    help="shortest synthetic clip (default: half of --synthetic-seconds); 2 with --synthetic-seconds 6 = a SLURP-like "
                         "ragged corpus of 2-6 s utterances")
    ap.add_argument("--synthetic-exact", action="store_true",
                    help="every synthetic clip lasts exactly --synthetic-seconds (default: lengths drawn U[0.5, 1] x that, SURVEY.md 8d)")
    ap.add_argument("--classes-file", default=None,
                    help="one intent label per line; default: the reference's 101 ALL_CLASSES shipped with the package")
    ap.add_argument("--do-normalize", action="store_true")
    ap.add_argument("--normalize-on-device", action="store_true",
                    help="with --do-normalize: run zero_mean_unit_var_norm on the GPU right after the H2D copy instead of in numpy")
    ap.add_argument("--loader-threads", type=int, default=8,
                    help="decode / synthesise the NEXT batches on this many host threads while the GPU encodes the current one "
                         "(the reference loads inside collate_fn with num_workers=0, …base…py:53-57,67); 0 = inline")
    ap.add_argument("--sink-threads", type=int, default=4, help="threads that wait for the D2H copies and write the per-utterance files")
    ap.add_argument("--text-prenet-state-dict", default="extracted/speecht5/mapping/text_prenet_state_dict.pickle")
    ap.add_argument("--tokenizer", default="microsoft/speecht5_asr",
                    help="-m text: name or local directory of the SpeechT5 tokenizer (the reference's processor, …base…py:38)")
    ap.add_argument("--format", choices=["pickle", "npy"], default="pickle")
    ap.add_argument("--gather", action="store_true", help="all-gather embeddings so that rank 0 writes everything")
    ap.add_argument("--inflight", type=int, default=0,
                    help="batches in flight on the GPU at once (each on its own stream / workspace / status block).  The batches "
                         "themselves are untouched -- the reference's pairs in corpus order -- and so are the results, bit for bit; "
                         "a pair of 5 s clips alone cannot fill 256 CUs.  1 = one batch at a time, as the reference runs; 0 (default) = "
                         "4 for utterances, 1 for --window-seconds >= 60 (a pair of 10-minute windows fills the chip by itself and "
                         "every slot would hold a 15 GB workspace)")
    ap.add_argument("--pack", type=int, default=0,
                    help="encode G of the reference's batches as ONE launch sequence (loco_forward_packed): the batches themselves are "
                         "untouched -- corpus-order pairs, every clip keeps the padded length of its own batch for GroupNorm, the "
                         "positional conv, positions and the key mask -- so the embeddings equal those of --inflight to the fp32 "
                         "summation order of the GEMMs (<= 5e-6 relative L2), not bit for bit.  0 (default) = off.  32 is a good value "
                         "for 2-6 s utterances; --inflight then counts packs (default 3, each on one stream)")
    ap.add_argument("--pack-window", type=int, default=8,
                    help="with --pack: batches are sorted by padded length inside windows of this many packs before they are packed "
                         "(which batches share a pack does not change any embedding; short batches just do not idle in long packs).  "
                         "8: rows computed per frame kept 1.05; larger windows pad less (~1.02 at 32) for the price of more decoded audio "
                         "held on the host -- on 10 000 files 8 / 16 / 32 measured 784-818 k / 813 k / 827 k frames/s: within the run-to-run spread")
    ap.add_argument("--gil-switch-ms", type=float, default=0.5,
                    help="sys.setswitchinterval for the run, in ms (CPython's default is 5): the thread that enqueues forwards gives the "
                         "interpreter lock up at every library call and, with a dozen loader / writer threads runnable, waits a switch "
                         "interval per thread to get it back; 0 = leave the interpreter's setting alone")
    ap.add_argument("--precision", choices=["f16x3", "f32", "f16x2"], default="f16x3",
                    help="arithmetic of the contractions (include/loco_asr.h, loco_set_precision): f16x3 (default) = three fp16 MFMAs per "
                         "fp32-class product, ~1e-6 of an fp64 evaluation; f32 = every contraction on the exact fp32 MFMA (2.7x slower); "
                         "f16x2 = weights rounded to fp16, ~9e-4: at the 1e-3 bar, not inside it")
    ap.add_argument("--range-policy", choices=["fp32", "raise", "off"], default="fp32",
                    help="a batch whose activations leave the range of the fp16 planes (f16x3 / f16x2) is run again on the exact-fp32 "
                         "kernels (fp32, default), refused with an error (raise), or not checked at all (off)")
    ap.add_argument("--window-seconds", type=float, default=0.0,
                    help="cut every recording into windows of this many seconds (10-minute windows for hour-long podcasts, "
                         "BASELINE.json configs[3]); each window is an independent unit written as <id>_w<k>")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join("extracted", "speecht5" if args.pretrained else "speecht5_base")
    if args.modality == "text" and (args.window_seconds > 0 or args.gather or args.resume or args.pretrained):
        raise SystemExit("-m text: --window-seconds / --gather / --resume / --pretrained apply to audio only")
    return args


def setup_rank(args):
    """(world size, rank, this rank's device, whether collectives are issued) from the launcher's environment; the process group."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    print(f"Extracting {args.modality} embeddings from SLURP {args.split} set using SpeechT5 (rank {rank}/{world})")
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: this extractor has no CPU path")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    print("Running on", device)
    # LOCO_FORCE_COLLECTIVE=1 under a launcher: create the process group and issue every collective even at world size 1, so that
    # a one-GPU box runs the real RCCL gather of --gather on device tensors (tests/test_gpu_rccl_world1.py)
    collective = world > 1 or (os.environ.get("LOCO_FORCE_COLLECTIVE") == "1" and "RANK" in os.environ)
    if collective:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)
        dp.FORCE_COLLECTIVE = world == 1
    return world, rank, device, collective


class WindowFetch:
    """fetch for --window-seconds: one decode per recording, sliced per window.  The cache of one decoded recording is not
    thread-safe: windows are prepared by ONE thread, in order."""

    def __init__(self, fetch, units):
        self.fetch, self.units, self.recording, self.audio = fetch, units, None, None

    def __call__(self, u):
        i, a, b = self.units[u]
        if i != self.recording:
            self.recording = self.audio = None
            self.recording, self.audio = i, self.fetch(i)
        return self.audio[a:b]


def learn_lengths(fetch, lengths):
    """``lengths``, or -- a corpus: unknown until decoded -- what one decoding pass finds; only for the flags that need them."""
    return lengths if any(lengths) else [len(fetch(i)) for i in range(len(lengths))]


def load_units(args, device):
    """(items, classes, fetch, lengths): (id, text, path, 16000, label) per unit -- a synthetic clip, an utterance of the SLURP
    split or, with --window-seconds, a window of one -- the intent labels, ``fetch(unit) -> samples``, and the units' lengths in
    samples (0 = unknown until decoded)."""
    classes = load_classes(args.classes_file)
    if args.synthetic:
        n = int(args.synthetic_seconds * 16000)
        frac = 0.5 if args.synthetic_min_seconds is None else min(1.0, max(0.0, args.synthetic_min_seconds / args.synthetic_seconds))
        lengths = [n] * args.synthetic if args.synthetic_exact else la.synth.mixed_lengths(args.synthetic, n, min_fraction=frac)
        order = sorted(classes)
        items = [(f"synthetic-{i:06d}", "", None, 16000, order[i % 101]) for i in range(args.synthetic)]
        fetch = lambda i, _lens=lengths: la.synth.clip(i, _lens[i])  # noqa: E731
    else:
        items = read_slurp_split(args.data_path, args.split)
        fetch = lambda i, _items=items: audio_io.load_audio_16k(_items[i][2], device)  # noqa: E731
        lengths = [0] * len(items)  # unknown until decoded
    if args.window_seconds > 0:
        # windows become the units: (id_wk, text, path, sr, label) with a fetch that slices the parent recording
        win = int(args.window_seconds * 16000)
        units = dp.window_units(learn_lengths(fetch, lengths), win)
        fetch = WindowFetch(fetch, units)
        items = [(f"{items[i][0]}_w{a // win:03d}", items[i][1], items[i][2], 16000, items[i][4]) for (i, a, b) in units]
        lengths = [b - a for (_, a, b) in units]
    return items, classes, fetch, lengths


def plan_batches(args, items, fetch, lengths, world, rank, collective):
    """(this rank's batches of unit indices, rounds, pack, packs): the reference's batches dealt round-robin or
    --bucket-by-length's, less what --resume finds written; rounds (and packs, with --pack G: a "round" is then one pack of up to
    G of this rank's batches) are equal on all ranks, so that collectives line up."""
    if args.bucket_by_length:
        lengths = learn_lengths(fetch, lengths)  # one decoding pass to learn the lengths
        shards = [dp.shard_units(lengths, world, r) for r in range(world)]
        my_batches = [shards[rank][a:a + args.batch_size] for a in range(0, len(shards[rank]), args.batch_size)]
        n_rounds = (max(len(s) for s in shards) + args.batch_size - 1) // args.batch_size
    else:  # the reference's batches: corpus order, whole batches dealt round-robin
        my_batches = dp.shard_batches(len(items), args.batch_size, world, rank)
        n_rounds = dp.rounds(len(items), args.batch_size, world)  # equal on all ranks: collectives line up
    if args.resume:
        if args.gather and collective:
            raise SystemExit("--resume with --gather: rank 0 writes other ranks' files, so a rank cannot tell which of ITS batches are done")
        folder = os.path.join(os.path.join(args.out, args.split), args.modality)
        done = lambda b: all(os.path.exists(sink_mod.embedding_path(folder, items[i][0], args.format)) for i in b)  # noqa: E731
        kept = [b for b in my_batches if not done(b)]
        print(f"--resume: {len(my_batches) - len(kept)} of {len(my_batches)} batches already written, {len(kept)} to encode")
        my_batches, n_rounds = kept, len(kept)
    pack = max(0, args.pack)
    if pack * args.batch_size > 512:
        raise SystemExit(f"--pack {pack} x --batch-size {args.batch_size} = {pack * args.batch_size} clips per launch sequence; the library takes "
                         "at most 512 (loco_max_pack_clips) -- and gains nothing beyond ~128 clips of utterance length")
    if pack and args.bucket_by_length:
        raise SystemExit("--pack keeps the reference's batches (it packs WHOLE batches); --bucket-by-length re-forms them: use one or the other")
    return my_batches, n_rounds, pack, ((n_rounds + pack - 1) // pack if pack else 0)


def batch_len(f):
    return max(len(c) for c in f) if isinstance(f, list) else int(f["input_values"].shape[1])


def batch_clips(f):
    return len(f) if isinstance(f, list) else int(f["input_values"].shape[0])


class Staging:
    """What the host does ahead of the GPU -- decode or synthesise, pad, mask, copy -- on its loader threads: ``batches()`` and
    ``packs()`` yield this rank's work in order, ``(unit indices, features on the device)`` per batch or ``(list of unit-index
    lists, packed tensors)`` per pack, and ``(indices, None)`` for every round in which this rank has run out of batches: an empty
    contribution keeps the collectives lined up."""

    def __init__(self, args, device, processor, encoder, fetch, my_batches, n_rounds, inflight, pack, n_packs):
        self.device, self.processor, self.encoder, self.fetch = device, processor, encoder, fetch
        self.my_batches, self.n_rounds, self.inflight, self.pack, self.n_packs = my_batches, n_rounds, inflight, pack, n_packs
        self.pack_window = max(1, args.pack_window)
        self.fused_pack = not (args.do_normalize and args.normalize_on_device)
        if pack:
            processor.pin_memory = False  # batches are copied into the pack's pinned buffer: their own staging need not be pinned
        # the window cache of one decoded recording is not thread-safe: windows are prepared by ONE thread, in order
        n = self.n_loaders = 0 if args.loader_threads <= 0 else (1 if args.window_seconds > 0 else args.loader_threads)
        # loader threads start on GPU 0: select the rank's GPU for anything they do there
        threads = lambda k: ThreadPoolExecutor(k, initializer=torch.cuda.set_device, initargs=(device,))  # noqa: E731
        self.pool = threads(n) if n > 0 else None
        self.clip_pool = threads(n) if n > 1 and args.batch_size >= 8 and args.window_seconds <= 0 else None
        self.pack_pool = threads(min(4, n)) if pack and n > 0 else None

    def close(self):
        for ex in (self.pool, self.clip_pool, self.pack_pool):
            if ex is not None:
                ex.shutdown()

    def clips_of(self, idx, pool=None):
        clips = list(pool.map(self.fetch, idx)) if pool is not None else [self.fetch(i) for i in idx]
        if any(torch.is_tensor(c) for c in clips):  # some files were resampled on the device: the whole batch is padded there
            clips = [c if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c)).to(self.device) for c in clips]
        return clips

    def padded(self, clips):
        """pad and mask the clips of ONE reference batch (SpeechT5FeatureExtractor, …base…py:51-65)"""
        return self.processor(audio=clips, sampling_rate=16000, return_tensors="pt", padding="longest")

    def host_batch(self, rnd):
        """Everything the host does for one batch: decode, pad, mask (pinned memory) -- run ahead of the GPU on worker threads,
        several BATCHES at a time (a batch of the reference is two clips: parallelism inside one would be two threads wide)."""
        idx = self.my_batches[rnd] if rnd < len(self.my_batches) else []
        if not idx:
            return idx, None
        # a reference batch is two clips: decoded one after the other, the parallelism is across batches; a throughput batch
        # (--batch-size 32: 32 files of 30 s) is decoded by its own pool, or the GPU waits for one thread to read 30 MB of audio
        clips = self.clips_of(idx, self.clip_pool if len(idx) >= 8 else None)
        # the H2D copies are enqueued HERE, by the loader thread (pinned source, non-blocking, the default stream): the thread that
        # enqueues forwards only waits for the future; forward_async orders its stream behind the default stream
        return idx, self.padded(clips).to(self.device)

    def batches(self):
        pool, n_rounds = self.pool, self.n_rounds
        ahead = max(2, 2 * self.inflight, self.n_loaders)  # batches being prepared while others are on the GPU
        pending = deque(pool.submit(self.host_batch, r) for r in range(min(ahead, n_rounds))) if pool else None
        for rnd in range(n_rounds):
            if pool:
                work = pending.popleft().result()
                if rnd + ahead < n_rounds:
                    pending.append(pool.submit(self.host_batch, rnd + ahead))
            else:
                work = self.host_batch(rnd)
            yield work

    def feats_for_pack(self, idx):
        """one reference batch for the pack stage: its decoded clips (host arrays: padded and packed in one go by
        processor.pack_clips), or -- some clip was resampled on the device, or the normaliser is deferred to the device -- the
        batch as the processor forms it"""
        clips = self.clips_of(idx)
        if self.fused_pack and not torch.is_tensor(clips[0]):
            return clips
        f = self.padded(clips)
        # the deferred normaliser (--normalize-on-device) runs per BATCH, before batches are packed
        return f.to(self.device) if getattr(self.processor, "normalize_on_device", False) else f

    def make_pack(self, fs):
        if all(isinstance(f, list) for f in fs):
            return self.processor.pack_clips(fs, self.device, self.encoder._lib.loco_output_frames)
        return self.encoder.pack_batches([self.padded(f) if isinstance(f, list) else f for f in fs], self.device)

    def packs(self):
        """--pack.  Three host stages run ahead of the GPU: (1) every reference batch is decoded, padded and masked BY ITSELF on
        the loader pool (it stays the batch the reference forms), two windows ahead; (2) when a window of pack_window packs has
        all its batches, they are sorted by padded length and cut into packs of G (dp.pack_windows, dp.cut_window); (3) each pack
        is laid out in pinned memory and crosses PCIe as one copy (encoder.pack_batches) on a small pool of its own, so that it
        does not queue behind the decoding of later windows."""
        pool, pack_pool, pack, my = self.pool, self.pack_pool, self.pack, self.my_batches
        bounds = dp.pack_windows(self.n_packs, self.pack_window)
        futs, submitted = {}, 0
        for w, (p0, p1) in enumerate(bounds):
            ahead_to = bounds[min(len(bounds) - 1, w + 2)][1] * pack  # decoding runs two windows ahead
            while pool and submitted < min(ahead_to, len(my)):
                futs[submitted] = pool.submit(self.feats_for_pack, my[submitted])
                submitted += 1
            lo, hi = min(len(my), p0 * pack), min(len(my), p1 * pack)
            feats = {i: (futs.pop(i).result() if pool else self.feats_for_pack(my[i])) for i in range(lo, hi)}
            groups, owed = dp.cut_window([batch_len(feats[i]) for i in range(lo, hi)], lo, p1 - p0, pack)
            order = [i for sel in groups for i in sel]
            if order:  # the window's largest pack sizes the slots' workspaces at their next (re)allocation
                self.encoder.reserve_workspace(sum(batch_clips(feats[i]) for i in order[-pack:]), batch_len(feats[order[-1]]) + 8)
            jobs, nxt = deque(), 0
            for _ in groups:
                # at most a handful of packs are being laid out at a time: each is two pinned buffers of tens of MB, and a whole
                # window's worth at once sends the pinned allocator to the driver (hipHostMalloc stalls every other HIP call)
                while nxt < len(groups) and len(jobs) < 5:
                    sel = groups[nxt]
                    meta, fs = [my[i] for i in sel], [feats[i] for i in sel]
                    jobs.append((meta, pack_pool.submit(self.make_pack, fs) if pack_pool else fs))
                    nxt += 1
                meta, job = jobs.popleft()
                yield meta, (job.result() if pack_pool else self.make_pack(job))
            feats = None
            for _ in range(owed):
                yield [], None  # this rank has run out of batches


def forwards(stage, prof, finish, t_loop):
    """The producing side of the loop: every staged batch or pack enqueued on the GPU, as (meta, BaseModelOutput / ticket / None).
    ``prof`` (LOCO_EXTRACT_PROFILE=1): seconds spent waiting for the staged batch, in the H2D copy, enqueueing, and in the
    hand-over to the consumer (or, without one, in ``finish``); printed once the last item has been handed over."""
    encoder, device, pack = stage.encoder, stage.device, stage.pack
    tick = time.perf_counter
    t_a = tick()
    for meta, feats in (stage.packs() if pack else stage.batches()):
        t_b = t_c = tick()
        if feats is None:
            res = None
        elif pack:
            res = encoder.forward_packed_async(packed=feats)
        else:
            on_dev = feats if feats["input_values"].is_cuda else feats.to(device)
            t_c = tick()
            res = encoder.forward_async(**on_dev) if stage.inflight > 1 else encoder(**on_dev)
        t_d = tick()
        yield meta, res
        if prof is not None:
            t_e = tick()
            for k, v in enumerate((t_b - t_a, t_c - t_b, t_d - t_c, t_e - t_d)):
                prof[k] += v
        t_a = tick()
    if prof is not None:
        print("consumer thread so far, s: waiting for forwards %.3f, gather / sink hand-over %.3f; loop so far %.3f s"
              % (finish.waited, finish.handed, tick() - t_loop))
        if getattr(encoder, "submit_profile", None):
            print("inside forward_async / forward_packed_async, s:", {k: round(v, 4) for k, v in encoder.submit_profile.items()})
        print("main thread, ms per %s: wait for the staged batch %.3f, H2D %.3f, enqueue %.3f, hand-over / finish %.3f"
              % (("pack" if pack else "batch",) + tuple(1e3 * v / max(1, stage.n_packs if pack else stage.n_rounds) for v in prof)))


class Finisher:
    """What follows a forward: the optional gather, then the sink -- in order, whatever finished first.  Counts the frames encoded,
    the gather rounds, and the consumer side's seconds: ``waited`` for forwards (+ range check), ``handed`` results to the gather /
    the sink."""

    def __init__(self, sink, gatherer, items, encode_labels, pack, rank, device):
        self.sink, self.gatherer, self.items, self.encode_labels = sink, gatherer, items, encode_labels
        self.pack, self.rank, self.device = pack, rank, device
        self.frames = self.gathers = 0
        self.waited = self.handed = 0.0

    def submit(self, idx, emb, **kw):
        self.sink.submit([self.items[i][0] for i in idx], emb, self.encode_labels([self.items[i][4] for i in idx]), **kw)

    def write_gathered(self, done):
        if self.rank == 0:
            for gid, e in done:
                self.submit([gid], e[None])

    def __call__(self, item):
        """item = (meta, res): meta = the unit indices of one batch, or (--pack) the list of such lists of one pack; res =
        BaseModelOutput / ticket / None."""
        meta, res = item
        t0 = time.perf_counter()
        emb, idx, rows = None, meta, None
        if self.pack:
            idx = [i for b in meta for i in b]
            if res is not None:
                res.result()
                emb, spans = res.packed_output()
                rows = [t for (_, nb, t) in spans for _ in range(nb)]
                self.frames += sum(nb * t for (_, nb, t) in spans)
        else:
            out = res.result() if hasattr(res, "result") else res
            if out is not None:
                emb = out.last_hidden_state
                self.frames += int(emb.shape[0]) * int(emb.shape[1])
        t1 = time.perf_counter()
        if self.gatherer is not None:
            self.write_gathered(self.gatherer.submit(emb, idx, rows, self.device))  # two collectives per round, both overlapped (dp.py)
            self.gathers += 1
        elif idx:
            self.submit(idx, emb, rows=rows, chunk=8 if self.pack else 0)
        self.waited += t1 - t0
        self.handed += time.perf_counter() - t1


def report(args, device, my_batches, finish, t_loop, inflight, pack, gatherer, world):
    n_mine, frames = sum(len(b) for b in my_batches), finish.frames
    print(f"Encoded {n_mine} utterances ({frames} frames, padded frames included) in {t_loop:.3f} s: "
          f"{n_mine / max(t_loop, 1e-9):.1f} utterances/s, {frames / max(t_loop, 1e-9):,.0f} frames/s "
          f"(--inflight {inflight}{f', --pack {pack}' if pack else ''})")
    stats = {"utterances": n_mine, "frames": frames, "seconds": t_loop, "inflight": inflight, "pack": pack,
             "gpu_gib_allocated_peak": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2),
             "gpu_gib_reserved_peak": round(torch.cuda.max_memory_reserved(device) / 2 ** 30, 2)}
    print(f"GPU memory: {stats['gpu_gib_allocated_peak']} GiB allocated at peak, {stats['gpu_gib_reserved_peak']} GiB reserved by the allocator")
    if gatherer is not None:
        import torch.distributed as dist
        print(f"Embedding gathers issued: {finish.gathers} rounds, {gatherer.collectives} collectives (backend {dist.get_backend()}, world size {world})")
        stats["gather_rounds"], stats["collectives"] = finish.gathers, gatherer.collectives
    return stats


def on_rank_device(device):
    """For a new host thread, which starts on GPU 0 and with autograd on: select the rank's GPU, and no_grad for the thread's life."""
    torch.cuda.set_device(device)
    torch.set_grad_enabled(False)


def main(argv=None):
    args = parse_args(argv)
    if args.gil_switch_ms > 0:
        sys.setswitchinterval(args.gil_switch_ms / 1000.0)
    world, rank, device, collective = setup_rank(args)
    items, classes, fetch, lengths = load_units(args, device)
    print(f"{args.split} set size: {len(items)}")
    encode_labels = one_hot_encoder(classes)
    if args.modality == "text":
        return extract_text(args, items, encode_labels, device, world, rank)

    model = load_model(args, device)
    processor = la.SpeechT5FeatureExtractorMI355X(do_normalize=args.do_normalize, pin_memory=True,
                                                  normalize_on_device=args.do_normalize and args.normalize_on_device)
    my_batches, n_rounds, pack, n_packs = plan_batches(args, items, fetch, lengths, world, rank, collective)
    inflight = args.inflight if args.inflight > 0 else (1 if args.window_seconds >= 60 else (3 if pack else 4))
    encoder = model.speecht5.encoder
    encoder.precision, encoder.range_policy = args.precision, args.range_policy
    if inflight > 1 or pack:
        encoder.set_inflight(max(1, inflight))
    if pack and inflight > 1:
        # packs in flight fill each other's tails: the two half-batch schedule INSIDE a forward (loco_set_streams) then only adds
        # launches -- measured at 32 pairs per pack: 820 k frames/s with two streams per pack and two packs in flight, 924 k with one
        # stream per pack, 944 k with three packs in flight (profiles/r04_packed_bench_streams.txt)
        encoder.streams = 1
    stage = Staging(args, device, processor, encoder, fetch, my_batches, n_rounds, inflight, pack, n_packs)
    gatherer = dp.RaggedGatherPipeline(cap=args.batch_size * max(1, pack)) if args.gather and collective else None

    torch.cuda.synchronize(device)
    t_loop = time.perf_counter()
    with torch.no_grad(), sink_mod.EmbeddingSink(args.out, args.split, args.modality, args.format, workers=args.sink_threads,
                                                 max_pending=max(4, 4 * inflight, 16 * (pack > 0))) as sink:
        finish = Finisher(sink, gatherer, items, encode_labels, pack, rank, device)
        prof = [0.0] * 4 if os.environ.get("LOCO_EXTRACT_PROFILE") == "1" else None
        # With batches in flight the consumer thread waits for each batch IN ORDER (an event, not a device-wide synchronisation),
        # checks its range status and hands it to the gather / the sink, while this thread stages (H2D) and enqueues forwards.
        failures = run_ordered(forwards(stage, prof, finish, t_loop), finish, inflight, threaded=inflight > 1 or bool(pack),
                               name="loco-finish", init=lambda: on_rank_device(device))
        if failures:
            if collective:
                # the other ranks are (or will be) blocked in this round's collectives: a rank that stops contributing must take the
                # job down, not leave it hanging -- the launcher (torchrun) tears the other ranks down when one exits non-zero
                traceback.print_exception(type(failures[0]), failures[0], failures[0].__traceback__)
                sys.stdout.flush()
                sys.stderr.flush()
                os._exit(13)
            raise failures[0]
        if gatherer is not None:
            finish.write_gathered(gatherer.flush())
    torch.cuda.synchronize(device)
    t_loop = time.perf_counter() - t_loop  # decode / synthesis -> batching -> encoder -> sink, files closed
    stats = report(args, device, my_batches, finish, t_loop, inflight, pack, gatherer, world)
    stage.close()
    print("Done!")
    if collective:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return stats


if __name__ == "__main__":
    main()
