"""-m gpu: the GPT-2 scorer end to end -- against HuggingFace in float64 (fixtures lm1 / lm2), the max_len walk against its per-window
calls, the per-recording fold and the CLI.

Bars: a GPU figure may be 4 x what HuggingFace's own fp32 run, stored in the same fixture, is away from float64 -- both are fp32 products
with fp32 accumulation over 768 / 3072 / 50 257 terms in different orders -- and the hidden states must also be within the project's
standing 2e-5.  The hidden-state figure is the relative L2 over the fixture's probe rows, the largest over the n_layer + 1 states."""
import importlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

import lm_ref
from conftest import GOLDEN, golden, record_figure

pytestmark = pytest.mark.gpu
la = importlib.import_module("loco-asr_amd")
lm = la.lm
eval_ppl = importlib.import_module("loco-asr_amd.eval_ppl")
_models = {}


def model_of(name):
    if name not in _models:
        g = golden(name + ".npz")
        sd = la.synth.gpt2_state_dict(int(g["seed"]), int(g["n_layer"]), int(g["n_positions"]), int(g["vocab"]), float(g["logit_scale"]))
        m = la.GPT2LMHeadModelMI355X.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, n_positions=int(g["n_positions"])).to("cuda")
        _models[name] = (g, sd, m)
    return _models[name]


@pytest.mark.parametrize("name", ["lm1", "lm2"])
def test_end_to_end_against_hf_float64(name):
    g, _, m = model_of(name)
    n_seq = int(g["n_seq"])
    ids = [g[f"ids{k}"] for k in range(n_seq)]
    # the three equal rows as one batch, the ragged set (5, 17, 64) as one right-padded batch
    nll = list(m.token_nll(torch.from_numpy(np.stack(ids[:3])).cuda()).double().cpu().numpy())
    ragged = m.token_nll_ragged([torch.from_numpy(t).cuda() for t in ids[3:]], batch_size=8)
    nll += [t.double().cpu().numpy() for t in ragged]
    nll_err = max(float(np.abs(a - g[f"nll{k}"]).max()) for k, a in enumerate(nll))
    hs = [m(torch.from_numpy(np.stack(ids[:3])).cuda(), output_hidden_states=True)]
    lens = [len(t) for t in ids[3:]]
    padded = np.zeros((len(lens), max(lens)), np.int64)
    for b, t in enumerate(ids[3:]):
        padded[b, :len(t)] = t
    hs.append(m(torch.from_numpy(padded).cuda(), output_hidden_states=True, lengths=lens))
    n_states = int(g["n_layer"]) + 1
    assert all(len(o.hidden_states) == n_states for o in hs) and hs[0].logits.shape == (3, 17, int(g["vocab"]))
    num, den = np.zeros(n_states), np.zeros(n_states)
    for k in range(n_seq):
        o, b = (hs[0], k) if k < 3 else (hs[1], k - 3)
        pos, probe = g[f"probe_pos{k}"], g[f"probe{k}"]
        for i in range(n_states):
            d = o.hidden_states[i][b].double().cpu().numpy()[pos] - probe[i]
            num[i] += (d ** 2).sum()
            den[i] += (probe[i] ** 2).sum()
    rel = np.sqrt(num / den)
    # the logits of the small-call path agree with the fused head's NLL
    z = hs[0].logits[0].double().cpu().numpy()
    via_logits = (np.log(np.exp(z[:-1] - z[:-1].max(-1, keepdims=True)).sum(-1)) + z[:-1].max(-1)) - z[np.arange(16), ids[0][1:]]
    hf_nll, hf_rel = float(g["hf_fp32_nll_max_abs_err"]), float(g["hf_fp32_hidden_rel_l2"].max())
    record_figure("lm_end_to_end", fixture=name, nll_max_abs_err=nll_err, hf_fp32_nll_max_abs_err=hf_nll, hidden_rel_l2=rel.tolist(),
                  hidden_rel_l2_max=float(rel.max()), hf_fp32_hidden_rel_l2_max=hf_rel, logits_vs_head=float(np.abs(via_logits - nll[0]).max()))
    print(name, "nll err", nll_err, "(HF fp32:", hf_nll, ") hidden rel l2", float(rel.max()), "(HF fp32:", hf_rel, ")")
    assert nll_err <= 4.0 * hf_nll
    assert rel.max() <= 4.0 * hf_rel and rel.max() <= 2e-5
    assert np.abs(via_logits - g["nll0"]).max() <= 4.0 * hf_nll


def test_token_nll_is_zero_beyond_a_rows_length_and_names_a_bad_id():
    g, _, m = model_of("lm2")
    ids = np.stack([g["ids0"], g["ids1"]])
    full = m.token_nll(torch.from_numpy(ids).cuda())
    cut = m.token_nll(torch.from_numpy(ids).cuda(), lengths=[17, 6])
    assert torch.equal(cut[0], full[0]) and torch.equal(cut[1, :5], full[1, :5]) and bool((cut[1, 5:] == 0).all())
    bad = ids.copy()
    bad[1, 4] = int(g["vocab"])
    with pytest.raises(ValueError, match=r"position 21 .*outside \[0, 1003\)"):
        m.token_nll(torch.from_numpy(bad).cuda())


def test_max_len_mode_equals_its_windows():
    """max_len = 16 on a 40-token recording (the 12-layer lm2 weights): the batched walk against one token_nll call per window, bit for
    bit; against the float64 restatement within the end-to-end bar; and the rows scored are the reference's: window 0 in full, every
    later window's last position, the final token never."""
    g, sd, m = model_of("lm2")
    n, W = 40, 16
    seq = la.synth.gpt2_token_ids(n, int(g["vocab"]), "max_len/recording")
    tokens = torch.from_numpy(seq.astype(np.int32)).cuda()
    got, targets = [], []
    for starts, first, last in lm.max_len_plan(n, W, bsize=5):
        rows = np.arange(W - 1) if first else np.arange(len(starts)) * W + (W - 2)
        got.append(m.nll_rows(tokens, starts, [W] * len(starts), W, rows))
        targets += list(range(1, W)) if first else [o + W - 1 for o in starts]
    got = torch.cat(got)
    assert targets == list(range(1, n - 1))                      # every token but the first and, the reference's quirk, the last
    per_window = [m.token_nll(tokens[None, :W].long())[0]]
    per_window += [m.token_nll(tokens[None, o:o + W].long())[0, -1:] for o in range(1, n - W)]
    assert torch.equal(got.view(torch.int32), torch.cat(per_window).view(torch.int32))
    ref = np.concatenate([lm_ref.token_nll(sd, seq[:W])] + [lm_ref.token_nll(sd, seq[o:o + W])[-1:] for o in range(1, n - W)])
    err = float(np.abs(got.double().cpu().numpy() - ref).max())
    record_figure("lm_max_len", max_abs_err=err, hf_fp32_nll_max_abs_err=float(g["hf_fp32_nll_max_abs_err"]), windows=n - W)
    assert err <= 4.0 * float(g["hf_fp32_nll_max_abs_err"])


def test_walk_of_the_window_fixture_and_the_device_fold(tmp_path):
    """score_max_len / score_indep on the lines of lm_windows.json: the recordings and the number of NLLs each gets are the fixture's, and
    the device fold (double, fixed order) is exp(mean) of exactly those NLLs."""
    with open(os.path.join(GOLDEN, "lm_windows.json")) as fh:
        fx = json.load(fh)
    _, _, m = model_of("lm2")
    p = tmp_path / "text"
    p.write_text("".join(f"{u} {t}\n" for u, t in fx["lines"]))
    utts = lm.read_key_text(str(p))
    tok = lm.TokenizedLines(eos_token_id=fx["eos"], bos_token_id=fx["bos"])
    want = {}
    for b in fx["max_len_batches"]:
        want[b["rec_ids"][0]] = want.get(b["rec_ids"][0], 0) + (len(b["batch"][0]) - 1 if b["first"] else len(b["batch"]))
    nlls, ppl = lm.score_max_len(m, utts, tok, bsize=fx["bsize"], max_len=fx["max_len"])
    assert {k: len(v) for k, v in nlls.items()} == want and "rC" not in ppl and set(ppl) == set(want)
    lifted, _ = lm.score_max_len(m, utts, tok, bsize=fx["bsize"], max_len=fx["max_len"], strict_reference=False)
    assert len(lifted["rC"]) == 7 and len(lifted["rE"]) == want["rE"] + 1 and lifted["rE"][:want["rE"]] == nlls["rE"]
    for r, v in nlls.items():
        assert abs(ppl[r] / float(np.exp(np.mean(np.asarray(v, np.float64)))) - 1.0) < 1e-12, r
    nlls_i, ppl_i = lm.score_indep(m, utts, tok, bsize=fx["bsize"])
    want_i = {}
    for u, b in zip(fx["indep"]["utt_ids"], [s for batch in fx["indep"]["batches"] for s in batch]):
        want_i[u.split("-")[0]] = want_i.get(u.split("-")[0], 0) + len(b) - 1
    assert {k: len(v) for k, v in nlls_i.items()} == want_i
    ref_rec, ref_ppl = lm_ref.fold([v for v in nlls_i.values()], [k + "-x" for k in nlls_i])
    assert all(abs(ppl_i[r] / ref_ppl[r] - 1.0) < 1e-12 for r in ppl_i)


def test_cli_writes_the_references_two_files(tmp_path):
    """eval_ppl --random-init --tokenized on 30 utterances of 3 recordings, both context modes."""
    V = 1003
    lines, want = [], {}
    for i in range(30):
        rec, n = f"rec{i % 3}", 2 + (i * 7) % 9
        ids = la.synth.gpt2_token_ids(n, V - 1, f"cli/{i}")
        lines.append(f"{rec}-A-{i:04d}00-{i:04d}99 " + " ".join(map(str, ids)))
        want[rec] = want.get(rec, 0) + n + 1
    src = tmp_path / "fisher.txt"
    src.write_text("\n".join(lines[::-1]) + "\n")
    common = ["--in_file", str(src), "--random-init", "--layers", "2", "--positions", "32", "--vocab", str(V), "--tokenized", "--bsize", "4"]
    for mode, count in (("indep", lambda n_tok: n_tok), ("max_len", lambda n_tok: n_tok - 2)):
        out = tmp_path / mode
        assert eval_ppl.main(common + ["--out_dir", str(out), "--context_type", mode]) == 0
        with open(out / "rec_id2nlls.pkl", "rb") as fh:
            nlls = pickle.load(fh)
        with open(out / "rec_id2ppl.json") as fh:
            ppl = json.load(fh)
        assert set(nlls) == set(ppl) == {"rec0", "rec1", "rec2"}
        for r in nlls:   # want = ids + one <eos> per utterance.  indep: <bos> ids <eos>, all but the last position; max_len: every token but the first and the last
            assert len(nlls[r]) == count(want[r]) and all(np.isfinite(nlls[r])), (mode, r)
            assert abs(ppl[r] / float(np.exp(np.mean(nlls[r]))) - 1.0) < 1e-9
        log = [f for f in os.listdir(out) if f.endswith(".log")]
        assert log == [f"gpt2_{mode}_fisher.log"] and "Avg. PPL of recordings:" in (out / log[0]).read_text()
