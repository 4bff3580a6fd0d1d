#!/usr/bin/env python3
"""What sampling costs, and that it costs greedy decoding nothing -> profiles/decoder_sample_cost.json (tools, not bench.py).

    python tools/decoder_sample_bench.py --parent PARENT_TREE        # PARENT_TREE: a checkout of the parent commit with its own
                                                                    # libloco_asr.so, as tools/decoder_parent_compare.py takes one

1. The regression rule.  The greedy pool step (loco_decoder_pool_step) with 64 open slots at T_enc = 249, all 6 decoder layers, timed in
   the parent tree and in this one, --reps processes each in alternation (a process loads one library).  The median of this tree's runs
   must lie inside the parent runs' range or below it; otherwise the file says by how much it does not, and the tool exits 1.  It also
   exits 1 when a slot closed during a timed greedy run (the poll block is read after every run).
2. Measured, no target.  In this tree's processes also loco_decoder_pool_step_sample on the same 64 slots, every slot drawing
   (temperature 0.8, top_p 0.95); then, in one process, tokens / s of sample_many at N = 4 against generate_many on the 512-utterance
   corpus of tools/decoder_pool_bench.py, --reps runs each in alternation.

    python tools/decoder_sample_bench.py steps TREE                  # one process of 1. and 2.: prints one JSON line
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, S = 64, 249, 450


def load(root):
    import torch
    sys.path.insert(0, root)
    la = importlib.import_module("loco-asr_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(la.__file__))) == root, la.__file__
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0))
    dsd, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(0))
    model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), decoder_state_dict=t(dsd), postnet_state_dict=t(post)).to("cuda")
    x, m = la.synth.batch([16000, 16000])
    model.generate(torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda(), max_length=4)  # loads the weights
    return la, model


def steps(root, n_steps, runs):
    """Per-step milliseconds of the greedy pool step and, where the tree has it, of the sampling step: `runs` timed runs of each."""
    import torch
    la, model = load(os.path.abspath(root))
    _libmod = importlib.import_module("loco-asr_amd._lib")
    lib, h = _libmod.load(), model.speecht5.encoder._handle
    p = lambda tn: C.c_void_p(tn.data_ptr())  # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    need = int(lib.loco_decoder_pool_workspace_bytes(h, B, T, S))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids, rows, caps = (C.c_int32 * B)(*range(B)), (C.c_int32 * B)(*[T] * B), (C.c_int32 * B)(*[S] * B)
    block = torch.zeros(4 + 2 * B, dtype=torch.int32).pin_memory()
    can_sample = hasattr(_libmod, "SampleConfig")
    cfg = _libmod.SampleConfig(C.sizeof(_libmod.SampleConfig), 0.8, 0, 0.95, 5) if can_sample else None

    def still_open():
        _libmod.check(lib.loco_decoder_pool_poll(h, B, T, S, p(block), p(ws), need, st()))
        torch.cuda.synchronize()
        return int(block[0])

    def run(sample):
        _libmod.check(lib.loco_decoder_pool_init(h, B, T, S, p(ws), need, st()))
        if sample:
            utts, hyps = (C.c_uint32 * B)(*range(B)), (C.c_uint32 * B)()
            _libmod.check(lib.loco_decoder_pool_admit_samples(h, B, T, S, B, 1, ids, p(enc_out), T * 768, rows, None, caps, utts, hyps, None, p(ws), need,
                                                              st()))
        else:
            _libmod.check(lib.loco_decoder_pool_admit(h, B, T, S, B, ids, p(enc_out), T * 768, rows, None, caps, p(ws), need, st()))
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n_steps):
            if sample:
                _libmod.check(lib.loco_decoder_pool_step_sample(h, B, T, S, i, T, C.byref(cfg), None, None, p(ws), need, st()))
            else:
                _libmod.check(lib.loco_decoder_pool_step(h, B, T, S, i, T, None, p(ws), need, st()))
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n_steps

    # with synthetic weights a row ends at its first token or never: draw encoder rows until every greedy slot outlives the timed steps
    for seed in range(16):
        enc_out = torch.randn((B, T, 768), device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
        run(False)
        if still_open() == B:
            break
    else:
        sys.exit("no draw of encoder rows keeps all 64 slots open")
    greedy, sampled, opens, opens_sampled = [], [], [], []
    for _ in range(runs):
        greedy.append(run(False))
        opens.append(still_open())
        if can_sample:
            sampled.append(run(True))
            opens_sampled.append(still_open())
    return dict(tree=root, encoder_rows_seed=seed, steps=n_steps, greedy_step_ms=greedy, slots_open_after_greedy_runs=opens,
                sample_step_ms=sampled, slots_open_after_sample_runs=opens_sampled)


def corpus_rates(reps, utterances):
    import torch
    la, model = load(ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from decoder_pool_bench import corpus, wall
    batches, caps = corpus(utterances)
    variants = {
        "generate_many_64_slots": lambda: sum(len(r) - 1 for r in model.generate_many(batches, max_length=caps, slots=64, pack=32)),
        "sample_many_N4_64_slots": lambda: sum(len(r) - 1 for per in model.sample_many(batches, num_return_sequences=4, temperature=0.8, top_p=0.95, seed=5, max_length=caps, slots=64,
                                                                                     pack=32) for r in per),
    }
    runs, tokens = {k: [] for k in variants}, {}
    for _ in range(reps):
        for k, fn in variants.items():
            s, n = wall(fn)
            runs[k].append(s)
            tokens[k] = n
            print(k, f"{s:.3f} s, {n} tokens", flush=True)
    torch.cuda.synchronize()
    return {k: dict(seconds=v, tokens=tokens[k], tokens_per_s=tokens[k] / min(v), utterances_per_s=utterances / min(v)) for k, v in runs.items()}


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "steps":
        print("RESULT " + json.dumps(steps(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 32, int(sys.argv[4]) if len(sys.argv) > 4 else 3)))
        return 0
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit with its own libloco_asr.so")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_sample_cost.json"))
    args = ap.parse_args()
    per_tree = {"parent": [], "new": []}
    for _ in range(args.reps):
        for name, tree in (("parent", os.path.abspath(args.parent)), ("new", ROOT)):
            try:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "steps", tree, str(args.steps), "3"], check=True, capture_output=True,
                                     text=True, timeout=300, cwd=tree).stdout
            except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:  # nothing more is started on the device
                print(f"the {name} tree's step process failed: {e}\n{getattr(e, 'stderr', '') or ''}", file=sys.stderr)
                return 3
            per_tree[name].append(json.loads(next(l for l in out.splitlines() if l.startswith("RESULT "))[7:]))
            print(name, per_tree[name][-1]["greedy_step_ms"], per_tree[name][-1]["sample_step_ms"], flush=True)
    flat = lambda name, key: [v for r in per_tree[name] for v in r[key]]  # noqa: E731
    parent, new, sampled = flat("parent", "greedy_step_ms"), flat("new", "greedy_step_ms"), flat("new", "sample_step_ms")
    # this tree's figure is the median of its runs: a best run below the parent's worst would pass a tree that is slower on the whole
    figure = statistics.median(new)
    inside = figure <= max(parent)
    opens = flat("parent", "slots_open_after_greedy_runs") + flat("new", "slots_open_after_greedy_runs")
    all_open = opens == [B] * len(opens)  # a slot that closed during a timed run made the later steps cheaper: the run does not count
    res = {"clock_state": "as found (not pinned)",
           "greedy_pool_step_B64_T249": dict(parent_ms=parent, new_ms=new, parent_range_ms=[min(parent), max(parent)], parent_median_ms=statistics.median(parent),
                                             new_median_ms=figure, new_best_ms=min(new), new_best_minus_parent_best_ms=min(new) - min(parent),
                                             rule="the median of this tree's runs lies inside the parent runs' range or below it",
                                             new_inside_parent_range_or_better=bool(inside), new_above_parent_range_ms=max(0.0, figure - max(parent)),
                                             processes_per_tree=args.reps, alternated=True, steps_per_run=args.steps,
                                             slots_open_after_each_run=opens, all_slots_open_after_every_run=all_open),
           "sample_pool_step_B64_T249": dict(ms=sampled, best_ms=min(sampled), minus_greedy_best_ms=min(sampled) - min(new), temperature=0.8, top_p=0.95, top_k=0,
                                             slots_open_after_each_run=flat("new", "slots_open_after_sample_runs")),
           "corpus": dict(utterances=args.utterances, caps="90 % in 10-60, 10 % at 450, Philox seed 5", reps=args.reps,
                          variants=corpus_rates(args.reps, args.utterances))}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0 if inside and all_open else 1


if __name__ == "__main__":
    sys.exit(main())
