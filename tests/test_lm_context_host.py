"""Host side of the language model's cached context: ``carry`` mode's plan against a restatement written from its rules, the plan's
invariants, the CLI's new flags, and what the C ABI and the Python API refuse before any launch.  No GPU."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

import lm_context_ref
from conftest import GOLDEN

la = importlib.import_module("loco-asr_amd")
lm = la.lm
_libmod = importlib.import_module("loco-asr_amd._lib")
eval_ppl = importlib.import_module("loco-asr_amd.eval_ppl")

CHUNKS = (1, 2, 31, 32, 33, 7, 64, 5)


def window_recordings():
    """utterance lengths (with <eos>) per recording of lm_windows.json: recordings of 3, 7, 8, 9 and 13 tokens"""
    with open(os.path.join(GOLDEN, "lm_windows.json")) as fh:
        fx = json.load(fh)
    utts = {}
    for u, t in fx["lines"]:
        utts.setdefault(u, t)
    lens = {}
    seqs = lm.recordings(utts, lm.TokenizedLines(eos_token_id=fx["eos"], bos_token_id=fx["bos"]), lens)
    assert sorted(len(s) for s in seqs.values()) == [3, 7, 8, 9, 13]
    assert all(sum(lens[r]) == len(seqs[r]) for r in seqs)
    return lens


def check_invariants(plan, chunk_lens, n_positions, keep):
    total = int(np.sum(chunk_lens))
    # every token is in exactly one chunk, in order: with the first token's NLL dropped, every token but the first is scored once
    assert [p[2] for p in plan] == [0] + [p[3] for p in plan[:-1]] and plan[-1][3] == total
    rebased_yet = False
    for base, P, a, b, rebased in plan:
        assert 0 <= base and P == a - base and P + (b - a) <= n_positions
        assert 1 <= b - a <= n_positions - keep     # an over-long utterance is split
        rebased_yet |= rebased
        if rebased:
            assert P == keep
        if rebased_yet:
            assert P >= keep                        # the left context of the chunk's first token; later tokens see more
        else:
            assert base == 0                        # before the first rebase: everything since the recording's start
    ctx = lm_context_ref.left_context(plan)
    assert sorted(ctx) == list(range(total)) and max(ctx.values()) <= n_positions - 1


@pytest.mark.parametrize("keep", [1, 16, 63])
def test_carry_plan_equals_its_restatement(keep):
    plan = list(lm.carry_plan(CHUNKS, 64, keep))
    assert plan == lm_context_ref.carry_plan(CHUNKS, 64, keep)
    check_invariants(plan, CHUNKS, 64, keep)
    assert any(p[4] for p in plan)
    # the 64-token utterance does not fit n_positions - keep and is split
    assert len(plan) > len(CHUNKS)
    assert sum(1 for p in plan if p[3] - p[2] == 64) == 0


def test_carry_plan_on_the_window_fixture():
    for rec, lens in window_recordings().items():
        plan = list(lm.carry_plan(lens, 8, 4))
        assert plan == lm_context_ref.carry_plan(lens, 8, 4), rec
        check_invariants(plan, lens, 8, 4)
        assert any(p[4] for p in plan) == (sum(lens) > 8), rec


def test_carry_plan_defaults_and_refusals():
    assert list(lm.carry_plan([3, 3], 8)) == list(lm.carry_plan([3, 3], 8, 4)) == [(0, 0, 0, 3, False), (0, 3, 3, 6, False)]
    assert list(lm.carry_plan([5, 5], 8, 2)) == [(0, 0, 0, 5, False), (3, 2, 5, 10, True)]
    for keep in (0, 8, -1):
        with pytest.raises(ValueError, match="keep"):
            list(lm.carry_plan([3], 8, keep))


def test_cli_takes_carry_and_keeps_its_defaults():
    p = eval_ppl.parser()
    a = p.parse_args(["-i", "x", "-o", "o", "--random-init", "--tokenized", "--context_type", "carry", "--keep", "16", "--inflight", "4"])
    assert (a.context_type, a.keep, a.inflight) == ("carry", 16, 4)
    a = p.parse_args(["-i", "x", "-o", "o", "--random-init"])
    assert (a.bsize, a.context_type, a.model, a.strict_reference, a.keep, a.inflight) == (128, "indep", "gpt2", True, None, 8)
    assert "strided perplexity" in " ".join(p.format_help().split())


def test_cabi_refuses_before_any_launch():
    lib = _libmod.load()
    assert not lib.loco_lm_cache_create(None, 4) and "null handle" in lib.loco_last_error().decode()
    h = lib.loco_lm_create(2, 64, 1003, 768, 12)
    assert h
    try:
        for slots in (0, -1, 65):
            assert not lib.loco_lm_cache_create(h, slots)
            assert "outside 1 .. 64" in lib.loco_last_error().decode()
        assert lib.loco_lm_ctx_workspace_bytes(h, 24, 3) > 0 and lib.loco_lm_ctx_workspace_bytes(h, 3 * 64, 3) > lib.loco_lm_ctx_workspace_bytes(h, 24, 3)
        for rows, N in ((24, 0), (24, 65), (2, 3), (3 * 64 + 1, 3), (-1, 1)):
            assert lib.loco_lm_ctx_workspace_bytes(h, rows, N) == 0, (rows, N)
        assert lib.loco_lm_ctx_workspace_bytes(None, 24, 3) == 0
        seqs = (C.c_int32 * 4)(0, 4, 0, 1)
        assert lib.loco_lm_ctx_step(h, None, None, seqs, 1, None, None, 0, None) == -1 and "null argument" in lib.loco_last_error().decode()
        assert lib.loco_lm_cache_reset(None, 0) == -1 and lib.loco_lm_cache_length(None, 0) == -1
        buf = (C.c_float * 16)()   # host memory stands in for the pointers: refused before a launch
        q = C.cast(buf, C.c_void_p)
        for seq3, N, word in (((0, 0, 0), 1, "len = 0"), ((4, 2, 0), 1, "slot = 2"), ((4, 0, 9), 1, "P = 9"), ((4, 0, 0), 0, "N = 0"), ((4, 0, 0), 65, "N = 65")):
            arr = (C.c_int32 * 3)(*seq3)
            assert lib.loco_op_lm_ctx_attention(q, q, q, 8 * 768, arr, N, 2, q, None) == -1
            assert word in lib.loco_last_error().decode(), word
        assert lib.loco_op_lm_ctx_attention(q, None, q, 768, (C.c_int32 * 3)(4, 0, 0), 1, 1, q, None) == -1
    finally:
        lib.loco_lm_destroy(h)
    assert lib.loco_abi_version() == 1


def test_python_refuses_cpu_tensors():
    sd = la.synth.gpt2_state_dict(0, 1, 8, 64)
    m = la.GPT2LMHeadModelMI355X.from_state_dict(sd)
    ids = torch.zeros(4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.new_cache(slots=2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.append(None, 0, ids)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.token_nll_given(None, [ids], slots=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lm.rescore(m, ids, [ids])
    with pytest.raises(ValueError, match="inflight"):
        lm.score_carry(m, {}, None, inflight=0)
