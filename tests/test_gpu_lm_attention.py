"""-m gpu: the cached-context attention kernel alone (loco_op_lm_ctx_attention, csrc/lm_attention.hip) against float64.

A call holds three ragged sequences on two cache slots; the visible set of query t of a sequence behind P cached tokens -- the slot's keys
j < P, its own keys t' <= t -- is restated for ``value_domain_cases.attention_ref`` as causal attention with offset P over the keys
[prefix | own].  P and L walk the kernel's paths: no prefix, a prefix of one key, one key short of / exactly / one key past half a key
tile, past a whole tile (65); sequences of 1, 2, 32, 33 and 70 queries (one lane, a full wave, a second wave, a second own key tile).  The
scores are planted (``value_domain_cases._planted``) so that the running maximum moves where the kernel is most likely to mishandle it:
at the last prefix key, at the first own key, at own key 31 / 32, and at every key (ascending).

The second half of the file repeats this with 1024 rows per slot: sequences of 129 .. 257 queries (a second and a third query tile of the
128 a workgroup owns) and prefixes of up to 1023 keys, the lead at own key 127 / 128 / 192, at prefix key 63 / 64 and at the last prefix key.

Bars are the project's own: per row 4 x torch's fp32 error against float64 (``row_bar``), and 1e-5 relative L2 (``BAR_ATTN``)."""
import ctypes as C

import numpy as np
import pytest
import torch

import value_domain_cases as vd
from conftest import record_figure

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    from gpu_util import check, dev, lib, ptr, rel_l2, stream

BAR_ATTN = 1e-5
PS = [0, 1, 31, 32, 33, 65]
LS = [70, 33, 32, 2, 1]
KINDS = ["last_prefix", "first_own", "own31", "own32", "ascending"]
CAP = 80  # rows per cache slot


def build(P_index, kind):
    """Three sequences: 0 and 2 on slot 0 behind P tokens, 1 on slot 1 behind the next P of the list.  Returns the packed q | k | v rows,
    the two slots' k and v planes and per sequence (len, slot, P)."""
    P0, P1 = PS[P_index], PS[(P_index + 1) % len(PS)]
    lens = [LS[(P_index + i) % len(LS)] for i in range(3)]
    seqs = [(lens[0], 0, P0), (lens[1], 1, P1), (lens[2], 0, P0)]
    g = torch.Generator().manual_seed(1000 * P_index + KINDS.index(kind))
    rows = sum(lens)
    q, k, u = vd._planted(g, rows, 2 * CAP + rows)       # keys: slot 0's rows, slot 1's rows, then every sequence's own
    q, k = q[0], k[0]
    v = torch.randn((2 * CAP + rows, 768), generator=g, dtype=torch.float64)
    base = float((vd.SCALE * torch.einsum("ihd,jhd->hij", q, k)).abs().max())
    lead = (vd.LEAD + 2 * base) * u
    own0 = 2 * CAP
    if kind == "ascending":
        step = vd.ASCENT / 64.0
        k = (0.2 * step / base) * k
        k[:2 * CAP] += step * torch.arange(CAP, dtype=torch.float64).repeat(2)[:, None, None] * u
    if kind == "last_prefix":                             # once per slot: sequences 0 and 2 share slot 0's keys
        for slot, P in ((0, P0), (1, P1)):
            if P:
                k[slot * CAP + P - 1] += lead
    for L, slot, P in seqs:
        if kind == "last_prefix":
            if P == 0:                                    # no prefix: the lead stands at the first own key instead
                k[own0] += lead
        elif kind == "first_own":
            k[own0] += lead
        elif kind in ("own31", "own32"):
            k[own0 + min(int(kind[3:]), L - 1)] += lead
        else:
            k[own0:own0 + L] += step * (P + torch.arange(L, dtype=torch.float64))[:, None, None] * u
        own0 += L
    qkv = torch.cat([q.reshape(rows, 768), k[2 * CAP:].reshape(rows, 768), v[2 * CAP:]], 1).float()
    kc, vc = k[:2 * CAP].reshape(2, CAP, 768).float(), v[:2 * CAP].reshape(2, CAP, 768).float()
    return qkv, kc, vc, seqs


def reference(qkv, kc, vc, seqs, dtype):
    out, r0 = [], 0
    for L, slot, P in seqs:
        own = qkv[r0:r0 + L]
        kk = torch.cat([kc[slot, :P], own[:, 768:1536]])[None]
        vv = torch.cat([vc[slot, :P], own[:, 1536:]])[None]
        out.append(vd.attention_ref(own[None, :, :768], kk, vv, None, 1, P, dtype)[0])
        r0 += L
    return torch.cat(out)


def launch(qkv, kc, vc, seqs, slots=2):
    rows = sum(s[0] for s in seqs)
    assert rows == qkv.shape[0]
    arr = (C.c_int32 * (3 * len(seqs)))(*[x for s in seqs for x in s])
    qd, kd, vd_ = dev(qkv), dev(kc), dev(vc)
    outs = []
    for _ in range(2):
        out = torch.full((rows, 768), float("nan"), device="cuda")
        check(lib().loco_op_lm_ctx_attention(ptr(qd), ptr(kd), ptr(vd_), kc.shape[1] * 768, arr, len(seqs), slots, ptr(out), stream()), "lm_ctx_attention")
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))      # two launches, the same bits
    return outs[0].cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P_index", range(len(PS)))
def test_prefix_plus_causal_against_float64(P_index, kind):
    qkv, kc, vc, seqs = build(P_index, kind)
    ref = reference(qkv, kc, vc, seqs, torch.float64)
    own = reference(qkv, kc, vc, seqs, torch.float32)
    out = launch(qkv, kc, vc, seqs)
    assert bool(torch.isfinite(out).all())
    bar = vd.row_bar(ref, own)
    fig = dict(rel_l2=rel_l2(out, ref), over_row_bar=vd.worst_ratio(out, ref, bar), max_abs=float((out.double() - ref).abs().max()),
               torch_fp32_max_abs=float((own.double() - ref).abs().max()))
    record_figure("lm_ctx_attention", kind=kind, seqs=seqs, **fig)
    print("lm ctx attention", kind, seqs, fig)
    assert fig["over_row_bar"] <= 1.0, fig
    assert fig["rel_l2"] <= BAR_ATTN, fig


def alone_among_others_and_moved(qkv, kc, vc, seqs):
    together = launch(qkv, kc, vc, seqs)
    r0 = 0
    for L, slot, P in seqs:
        alone = launch(qkv[r0:r0 + L], kc, vc, [(L, slot, P)])
        assert torch.equal(alone.view(torch.int32), together[r0:r0 + L].view(torch.int32)), (L, slot, P)
        # the slot's contents moved to slot index 2 of a wider cache, the sequence last of a call instead of first
        kc3, vc3 = torch.cat([kc, kc[slot:slot + 1]]), torch.cat([vc, vc[slot:slot + 1]])
        moved = launch(torch.cat([qkv[:5], qkv[r0:r0 + L]]), kc3, vc3, [(5, 1, 0), (L, 2, P)], slots=3)
        assert torch.equal(moved[5:].view(torch.int32), together[r0:r0 + L].view(torch.int32)), (L, slot, P)
        r0 += L


@pytest.mark.parametrize("P_index", [0, 3, 5])
def test_a_sequence_alone_is_itself_among_others_and_on_another_slot(P_index):
    qkv, kc, vc, seqs = build(P_index, "ascending")
    together = launch(qkv, kc, vc, seqs)
    r0 = 0
    for L, slot, P in seqs:
        alone = launch(qkv[r0:r0 + L], kc, vc, [(L, slot, P)])
        assert torch.equal(alone.view(torch.int32), together[r0:r0 + L].view(torch.int32)), (L, slot, P)
        # the slot's contents moved to slot index 2 of a wider cache, the sequence last of a call instead of first
        kc3, vc3 = torch.cat([kc, kc[slot:slot + 1]]), torch.cat([vc, vc[slot:slot + 1]])
        moved = launch(torch.cat([qkv[:5], qkv[r0:r0 + L]]), kc3, vc3, [(5, 1, 0), (L, 2, P)], slots=3)
        assert torch.equal(moved[5:].view(torch.int32), together[r0:r0 + L].view(torch.int32)), (L, slot, P)
        r0 += L


# ---- GPT-2's own lengths: 1024 rows per slot, more than one query tile ----------------------------------------------------------------------
# A workgroup owns 128 queries of one sequence.  Case A puts a second and a third query tile (q0 = 128, 256; own key tiles past the
# second; the skip of own tiles past a wave's last query; own_end = min(len, q0 + 128)) behind a prefix of exactly one key tile and of a
# single key; case B puts a second query tile of two queries, a half tile and a lone query behind 14 .. 16 prefix tiles, up to P = 1023
# and P + L = 1024, with two sequences of different P on one slot.
LONG_CAP = 1024
LONG_CASES = {"A": [(129, 0, 64), (257, 1, 1), (200, 0, 64)], "B": [(130, 0, 893), (64, 1, 960), (1, 0, 1023)]}
LONG_KINDS = ["own127", "own128", "own192", "prefix63", "prefix64", "last_prefix", "ascending"]


def build_long(case, kind):
    """The layout of ``build`` with LONG_CAP rows per slot.  The lead -- the key that outscores all others by about LEAD nats, where the
    running maximum arrives -- stands at own key 127 (the last of the first query tile), 128 (the first of the second), 192 (the first of
    the fourth own key tile), each clipped to the sequence's last key; at prefix key 63 or 64 of both slots (the last of the first key
    tile, the first of the second), clipped to the slot's last visible key; or at every sequence's last prefix key.  ascending: every key
    of the prefix, then every own key, raises the maximum."""
    seqs = LONG_CASES[case]
    g = torch.Generator().manual_seed(5000 + 100 * sorted(LONG_CASES).index(case) + LONG_KINDS.index(kind))
    rows = sum(s[0] for s in seqs)
    q, k, u = vd._planted(g, rows, 2 * LONG_CAP + rows)   # keys: slot 0's rows, slot 1's rows, then every sequence's own
    q, k = q[0], k[0]
    v = torch.randn((2 * LONG_CAP + rows, 768), generator=g, dtype=torch.float64)
    base = float((vd.SCALE * torch.einsum("ihd,jhd->hij", q, k)).abs().max())
    lead = (vd.LEAD + 2 * base) * u
    if kind == "ascending":
        step = vd.ASCENT / 64.0
        k = (0.2 * step / base) * k
        k[:2 * LONG_CAP] += step * torch.arange(LONG_CAP, dtype=torch.float64).repeat(2)[:, None, None] * u
    elif kind.startswith("prefix"):
        for slot in (0, 1):
            k[slot * LONG_CAP + min(int(kind[6:]), min(P for _, s, P in seqs if s == slot) - 1)] += lead
    elif kind == "last_prefix":
        for slot, P in sorted({(s, P) for _, s, P in seqs}):
            k[slot * LONG_CAP + P - 1] += lead
    own0 = 2 * LONG_CAP
    for L, slot, P in seqs:
        if kind.startswith("own"):
            k[own0 + min(int(kind[3:]), L - 1)] += lead
        elif kind == "ascending":
            k[own0:own0 + L] += step * (P + torch.arange(L, dtype=torch.float64))[:, None, None] * u
        own0 += L
    qkv = torch.cat([q.reshape(rows, 768), k[2 * LONG_CAP:].reshape(rows, 768), v[2 * LONG_CAP:]], 1).float()
    kc, vc = k[:2 * LONG_CAP].reshape(2, LONG_CAP, 768).float(), v[:2 * LONG_CAP].reshape(2, LONG_CAP, 768).float()
    return qkv, kc, vc, seqs


@pytest.mark.parametrize("kind", LONG_KINDS)
@pytest.mark.parametrize("case", sorted(LONG_CASES))
def test_later_query_tiles_and_long_prefixes_against_float64(case, kind):
    qkv, kc, vc, seqs = build_long(case, kind)
    assert all(P + L <= LONG_CAP for L, _, P in seqs)
    ref = reference(qkv, kc, vc, seqs, torch.float64)
    own = reference(qkv, kc, vc, seqs, torch.float32)
    out = launch(qkv, kc, vc, seqs)                       # two launches, the same bits
    assert bool(torch.isfinite(out).all())
    bar = vd.row_bar(ref, own)
    fig = dict(rel_l2=rel_l2(out, ref), over_row_bar=vd.worst_ratio(out, ref, bar), max_abs=float((out.double() - ref).abs().max()),
               torch_fp32_max_abs=float((own.double() - ref).abs().max()))
    record_figure("lm_ctx_attention_long", case=case, kind=kind, seqs=seqs, bar_rel_l2=BAR_ATTN, **fig)
    print("lm ctx attention long", case, kind, seqs, fig)
    assert fig["over_row_bar"] <= 1.0, fig
    assert fig["rel_l2"] <= BAR_ATTN, fig


def test_a_long_sequence_alone_is_itself_among_others_and_on_another_slot():
    alone_among_others_and_moved(*build_long("A", "ascending"))
