"""Beam search in the decoder slot pool (csrc/decoder_beam.hip) on the GPU.

1. loco_op_beam_select against tests/decoder_beam_ref.py, exact in every array the device keeps (tokens, parents, finished lists,
   flags, doubles bit for bit).  The restatement is fed the log-probabilities the operator hands out; those are compared separately
   against a float64 log-softmax with the bar of tests/test_gpu_decoder_score.py.  Every buffer sits between guard bands.
2. loco_op_beam_reorder against numpy indexing, byte for byte.
3. The model (2 + 2 layers, weights whose rows end at different steps): ``beam_search_many`` replayed through the restatement on the
   log-probabilities the pool's steps used; the same bits at other ``slots``, in reversed order and beside a 30 s clip;
   ``num_beams=1`` against ``generate_many``; greedy unchanged by a beam call on the same handle.
4. Cache consistency: every hypothesis teacher-forced through ``model.score``; the bar is 4 x what greedy ``generate_many`` against
   ``model.score`` shows on the same clips in the same run.
5. ``beam_search``'s layout and the command line.
"""
import ctypes as C
import importlib
import json

import numpy as np
import pytest
import torch

import decoder_beam_ref as ref
import decoder_pool_cases as pc
from conftest import record_figure
from test_gpu_decoder_pool import batches_of
from test_gpu_decoder_score import GAP, floor_of

pytestmark = pytest.mark.gpu

GUARD = 64  # elements on either side of every buffer


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


def beam_config(gu, K, length_penalty=1.0, early=0):
    return gu._libmod.BeamConfig(C.sizeof(gu._libmod.BeamConfig), K, float(length_penalty), int(ref.EARLY.get(early, early)), 0)


def den_host(gu, length_penalty, n):
    d = np.zeros(n, np.float64)
    gu.check(gu.lib().loco_beam_den_table(float(length_penalty), n, d.ctypes.data_as(C.POINTER(C.c_double))), "loco_beam_den_table")
    assert np.array_equal(d.view(np.int64), ref.den_table(length_penalty, n).view(np.int64))  # the same pow as Python's **
    return d


class Guarded:
    """A host array on the device between two bands of a sentinel byte; ``back()`` checks the bands and returns the middle."""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.shape, self.dtype = a.shape, a.dtype
        raw = np.full(a.nbytes + 2 * GUARD * a.itemsize, 0xA5, np.uint8)
        raw[GUARD * a.itemsize:GUARD * a.itemsize + a.nbytes] = a.reshape(-1).view(np.uint8)
        self.t = torch.from_numpy(raw).cuda()
        self.off, self.nbytes = GUARD * a.itemsize, a.nbytes

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.off)

    def back(self):
        raw = self.t.cpu().numpy()
        assert bool((raw[:self.off] == 0xA5).all()) and bool((raw[self.off + self.nbytes:] == 0xA5).all()), "a guard band was written"
        return raw[self.off:self.off + self.nbytes].view(self.dtype).reshape(self.shape).copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def select_op(gu, groups, logits, ld, cfg, den, poll=True):
    """One loco_op_beam_select step on the state of ``groups`` (ref.BeamGroup, equal K / V / S): ({array name: host array over all
    groups}, logprobs f32 [G K, V], poll)."""
    G, K, V, S = len(groups), groups[0].K, groups[0].V, groups[0].S
    cat = lambda name: np.concatenate([getattr(g, name) for g in groups])  # noqa: E731
    st = {n: Guarded(cat(n)) for n in ref.BeamGroup.ARRAYS if n not in ("parent", "count")}
    st["parent"] = Guarded(np.full(G * K, -77, np.int32))
    st["count"] = Guarded(np.full(G * K, -77, np.int32))
    x = Guarded(np.asarray(logits, np.float32))
    lp = Guarded(np.full((G * K, V), 123.0, np.float32))
    pl = Guarded(np.full(1, -7, np.int32))
    d = Guarded(den)
    gu.check(gu.lib().loco_op_beam_select(
        x.ptr, ld, G, V, S, C.byref(cfg), d.ptr, st["status"].ptr, st["pos"].ptr, st["caps"].ptr, st["cur"].ptr, st["cnt"].ptr, st["lengths"].ptr,
        st["tokens"].ptr, st["tlp"].ptr, st["run"].ptr, st["alive"].ptr, st["unsat"].ptr, st["fin_n"].ptr, st["fin_score"].ptr, st["fin_sum"].ptr,
        st["fin_len"].ptr, st["fin_tok"].ptr, st["fin_tlp"].ptr, lp.ptr, st["parent"].ptr, st["count"].ptr, pl.ptr if poll else None, gu.stream()),
        "loco_op_beam_select")
    torch.cuda.synchronize()
    assert same_bits(x.back(), np.asarray(logits, np.float32)) and same_bits(d.back(), den)  # only read
    return {n: v.back() for n, v in st.items()}, lp.back(), int(pl.back()[0])


def step_and_compare(gu, groups, rows, cfg, den, pad=7):
    """One step of the operator and of the restatement on the operator's log-probabilities; every array must agree bit for bit.
    ``rows`` f32 [G K, V].  Returns the log-probabilities."""
    G, K, V = len(groups), groups[0].K, groups[0].V
    ld = V + pad
    x = np.full((G * K, ld), GAP, np.float32)
    x[:, :V] = rows
    was_open = [g.open for g in groups]
    before = {n: np.concatenate([getattr(g, n) for g in groups]) for n in ref.BeamGroup.ARRAYS}
    got, lp, poll = select_op(gu, groups, x, ld, cfg, den)
    for i, g in enumerate(groups):
        took = g.step(lp[i * K:(i + 1) * K])
        assert took == (was_open[i] and 0 <= before["pos"][i * K] < g.S - 1)
    for n in ref.BeamGroup.ARRAYS:
        want = np.concatenate([getattr(g, n) + (i * K if n == "parent" else 0) for i, g in enumerate(groups)]).astype(before[n].dtype)
        if n in ("parent", "count"):  # step outputs: a group that is not open leaves them as they were
            keep = np.repeat([not o for o in was_open], K)
            want = np.where(keep, -77, want).astype(np.int32)
        assert same_bits(got[n], want), (n, got[n], want)
    # a group that is not open: its log-probability rows are not written either
    for i, o in enumerate(was_open):
        if not o:
            assert bool((lp[i * K:(i + 1) * K] == 123.0).all())
    assert poll == sum(int(g.open) * K for g in groups)
    return lp


def check_logprobs(lp, rows):
    """The operator's rows against a float64 log-softmax: the bar of test_gpu_decoder_score (4 x torch fp32's own error, floor 2^-21)."""
    x = torch.from_numpy(np.asarray(rows, np.float32))
    want, own, got = torch.log_softmax(x.double(), -1), torch.log_softmax(x, -1), torch.from_numpy(lp).double()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(own))
    assert torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)])  # -inf stays -inf
    e_torch = float((own.double() - want)[fin].abs().max()) if bool(fin.any()) else 0.0
    bar = torch.maximum(torch.full_like(want, 4 * e_torch), floor_of(want))
    ratio = ((got - want).abs() / bar)[fin]
    assert not ratio.numel() or float(ratio.max()) <= 1.0, float(ratio.max())


WIDTHS = [32, 63, 64, 65, 81, 129, 1000]
BEAMS = [1, 2, 3, 5, 8, 16]
PARAMS = [(1.0, False), (0.0, True), (2.0, "never"), (1.0, True), (0.0, "never"), (2.0, False)]


# ---- 1. the select operator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", [(V, K) for V in WIDTHS for K in BEAMS if 2 * K <= V])
def test_select_op_sequences(gu, V, K):
    """Groups of different caps through a scripted run of steps -- the first step (one beam alive), a step in which every beam's best
    token is </s> (all of the top K hit), a step of identical rows with -inf columns, a step with a NaN row, steps at the caps --
    compared after every step.  Groups finish at different steps and then must be left alone; one group is never opened."""
    S = 9
    rng = np.random.default_rng(1000 * V + K)
    for n, G in enumerate(sorted({1, 3, 64 // K})):
        length_penalty, early = PARAMS[(n + K + V) % len(PARAMS)]
        cfg, den = beam_config(gu, K, length_penalty, early), den_host(gu, length_penalty, S)
        groups = [ref.BeamGroup(K, V, S, cap=4 + (g % 5), length_penalty=length_penalty, early_stopping=early, den=den) for g in range(G)]
        if G >= 3:  # never opened: status free and a state nobody initialised
            groups[1].status[:] = ref.FREE
            groups[1].fin_n[0], groups[1].pos[:] = 1 << 30, 3
        events = set()
        for j in range(8):
            rows = (rng.standard_normal((G * K, V)) * 4.0).astype(np.float32)
            if j == 0:
                rows[:, ref.EOS] -= 60.0  # the first step ends no hypothesis: K beams are alive after it
            elif j == 1:
                rows[:, ref.EOS] += 60.0  # every alive beam's best candidate is </s>
            elif j == 2:
                rows[:] = rows[0]
                rows[:, 5::7] = -np.inf
            elif j == 3 and K > 1:
                rows[1::K] = np.nan
            else:
                rows[:, ref.EOS] += rng.uniform(-2.0, 6.0)
            lp = step_and_compare(gu, groups, rows, cfg, den)
            took = np.repeat([int(g.lengths[0]) == j + 2 for g in groups], K)  # the groups that took step j
            if j != 3:
                check_logprobs(lp[took], rows[took])
            if j == 1:
                for g in groups:
                    if int(g.lengths[0]) == 3:  # its K beams were alive and every one's best candidate hit: K entries
                        assert int(g.fin_n[0]) == K
                        events.add("all_hit")
            events |= {"finished" for g in groups if not g.open and g.status[0] == ref.FINISHED}
        assert "all_hit" in events and "finished" in events
        assert not any(g.open for g in groups if g.status[0] != ref.FREE)  # cap <= 8: every opened group has ended


def test_select_op_ties_go_to_the_lower_flat_index(gu):
    K, V, S = 3, 32, 6
    cfg, den = beam_config(gu, K), den_host(gu, 1.0, S)
    g = ref.BeamGroup(K, V, S, cap=6, den=den)
    g.alive[:], g.run[:], g.pos[:] = 1, -1.5, 1
    g.tokens[:, 1], g.cur[:], g.cnt[:] = [7, 8, 9], [7, 8, 9], 2
    row = np.zeros(V, np.float32)
    row[[11, 20]] = [3.0, 3.0]  # two equal best columns in three equal rows: candidates (0,11) (0,20) (1,11) (1,20) (2,11) (2,20)
    step_and_compare(gu, [g], np.tile(row, (K, 1)), cfg, den)
    assert g.parent.tolist() == [0, 0, 1] and g.tokens[:, 2].tolist() == [11, 20, 11]
    assert g.run[0] == g.run[1] == g.run[2]


@pytest.mark.parametrize("early", [False, True, "never"])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
def test_select_op_full_list(gu, early, length_penalty):
    """A list that holds K entries before the step, in each value of early_stopping and length_penalty: once with a running beam
    that can still beat the list's worst entry and once with one that cannot (the flag falls and the group ends); a NaN score in the
    list sorts last."""
    K, V, S = 4, 81, 12
    cfg, den = beam_config(gu, K, length_penalty, early), den_host(gu, length_penalty, S)
    rng = np.random.default_rng(17)
    for worst, nan_entry in [(-50.0, False), (-0.001, False), (-50.0, True)]:
        groups = []
        for cap in (12, 7):  # far from the cap, and the step at the cap (cur + 1 == cap)
            g = ref.BeamGroup(K, V, S, cap=cap, length_penalty=length_penalty, early_stopping=early, den=den)
            g.alive[:], g.pos[:], g.cnt[:] = 1, 5, 6
            g.run[:] = [-3.0, -3.5, -4.0, -9.0]
            g.tokens[:, 1:6] = rng.integers(4, V, (K, 5))
            g.cur[:] = g.tokens[:, 5]
            g.tlp[:, 1:6] = -rng.random((K, 5)).astype(np.float32)
            g.fin_n[0] = K
            g.fin_score[:] = [-0.5, -0.75, -1.0, worst]
            if nan_entry:
                g.fin_score[3] = np.nan
            g.fin_sum[:], g.fin_len[:] = g.fin_score * 3, [3, 4, 4, 5]
            g.fin_tok[:, :5], g.fin_tlp[:, :5] = rng.integers(4, V, (K, 5)), -rng.random((K, 5)).astype(np.float32)
            groups.append(g)
        rows = (rng.standard_normal((2 * K, V)) * 2.0).astype(np.float32)
        rows[0, ref.EOS] += 8.0  # beam 0's </s> is the best candidate: it enters a list that takes entries
        step_and_compare(gu, groups, rows, cfg, den)
        if early is True:
            assert all(not g.open for g in groups) and groups[0].fin_score[0] == -0.5  # the full list is closed and the group done
        elif worst == -50.0:
            assert groups[0].fin_n[0] == K and groups[0].fin_len.tolist().count(7) >= 1  # the new entry (7 tokens) displaced one
        assert not groups[1].open  # at the cap nothing continues


def test_select_op_nan_rows_order_last(gu):
    K, V, S = 3, 32, 6
    cfg, den = beam_config(gu, K), den_host(gu, 1.0, S)
    g = ref.BeamGroup(K, V, S, cap=6, den=den)
    g.alive[:], g.run[:], g.pos[:], g.cnt[:] = 1, [-1.0, -0.5, -2.0], 1, 2
    rows = np.random.default_rng(3).standard_normal((K, V)).astype(np.float32)
    rows[1] = np.nan  # the beam with the best score so far: all of its candidates order after every number
    step_and_compare(gu, [g], rows, cfg, den)
    assert 1 not in g.parent.tolist() and g.alive.tolist() == [1, 1, 1]
    g2 = ref.BeamGroup(K, V, S, cap=6, den=den)  # only NaN candidates: they order by flat index, and the score compare ends the group
    step_and_compare(gu, [g2], np.full((K, V), np.nan, np.float32), cfg, den)
    assert g2.tokens[:, 1].tolist()[:2] == [0, 1] and not g2.open


def test_select_op_refusals(gu):
    lib = gu.lib()
    x = torch.zeros(64, device="cuda")
    args = lambda cfg, V=8: (gu.ptr(x), V, 1, V, 4, C.byref(cfg)) + (gu.ptr(x),) * 21 + (None, gu.stream())  # noqa: E731
    for cfg, V, word in [(beam_config(gu, 0), 8, "num_beams"), (beam_config(gu, 17), 64, "num_beams"), (beam_config(gu, 5), 9, "num_beams"),
                         (beam_config(gu, 2, float("inf")), 8, "length_penalty"), (beam_config(gu, 2, 1.0, 3), 8, "early_stopping")]:
        assert lib.loco_op_beam_select(*args(cfg, V)) == -1 and word in lib.loco_last_error().decode()
    bad = beam_config(gu, 2)
    bad.struct_size = 8
    assert lib.loco_op_beam_select(*args(bad)) == -1 and "struct_size" in lib.loco_last_error().decode()


# ---- 2. the reorder operator ----------------------------------------------------------------------------------------------------------
MAPPINGS = {"identity": lambda K: list(range(K)), "swap": lambda K: [1, 0] + list(range(2, K)), "cycle": lambda K: [1, 2, 0] + list(range(3, K)),
            "all_from_one": lambda K: [K - 1] * K, "outside": lambda K: [-5, 1 << 20] + list(range(2, K))}


def reorder_ref(buf, parents, counts, status, K):
    L, slots, S, W = buf.shape
    out = buf.copy()
    for r in range(slots):
        lo = r // K * K
        par = min(max(int(parents[r]), lo), min(lo + K - 1, slots - 1))
        if par == r or (status is not None and status[r] != 1):
            continue
        n = min(max(int(counts[r]), 0), S)
        out[:, r, :n] = buf[:, par, :n]
    return out


@pytest.mark.parametrize("slots,S,W,K", [(8, 5, 1536, 4), (8, 450, 1536, 4), (64, 5, 4, 4), (64, 450, 6, 16), (64, 450, 1, 3), (8, 450, 1, 3)])
def test_reorder_op(gu, slots, S, W, K):
    L = 2
    rng = np.random.default_rng(slots * S + W)
    buf = rng.integers(0, 2 ** 32, (L, slots, S, W), dtype=np.uint32)
    names = list(MAPPINGS)
    groups = (slots + K - 1) // K
    for call, count in enumerate([1, 63, 64, 65]):
        parents, counts = np.zeros(slots, np.int32), np.zeros(slots, np.int32)
        for g in range(groups):
            m = MAPPINGS[names[(g + call) % len(names)]](K)
            for k in range(K):
                if g * K + k < slots:
                    parents[g * K + k] = (g * K + m[k]) if 0 <= m[k] < K else m[k]
                    counts[g * K + k] = count + (k % 2) * (call % 2)  # siblings with different counts
        status = None
        if call == 2:  # a group that is not open does not move
            status = np.ones(slots, np.int32)
            status[:K] = 2
            counts[-1] = -3  # and a negative count moves nothing
        b, sh = Guarded(buf), Guarded(np.zeros_like(buf))
        p, c = Guarded(parents), Guarded(counts)
        st = Guarded(status) if status is not None else None
        gu.check(gu.lib().loco_op_beam_reorder(b.ptr, sh.ptr, L, slots, S, W, p.ptr, c.ptr, st.ptr if st else None, K, int(max(counts.max(), 0)),
                                               gu.stream()), "loco_op_beam_reorder")
        torch.cuda.synchronize()
        sh.back()
        want = reorder_ref(buf, parents, counts, status, K)
        assert same_bits(b.back(), want), (call, count)
        assert same_bits(p.back(), parents) and same_bits(c.back(), counts)
        buf = want


# ---- 3. the model ------------------------------------------------------------------------------------------------------------------------
K_MODEL = 4
CLIPS = 6
CAPS = [16, 12, 3, 24, 6, 4]  # two short enough that hypotheses end by the cap
_cache = {}


def beam_model(gu, beta=3.0):
    """2 + 2 layers; lm_head = 0.05 * embed, untied, with a constant ``beta`` on the </s> logit (decoder_beam_ref.beam_weights)."""
    if "model" not in _cache:
        la = gu.la
        pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0, pc.ENC_LAYERS))
        dec, post = la.synth.split_decoder_state_dict(ref.beam_weights(la.synth, beta, layers=pc.DEC_LAYERS))
        t = lambda d: {k: torch.from_numpy(np.array(v)) for k, v in d.items()}  # noqa: E731
        _cache["model"] = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), layers=pc.ENC_LAYERS, decoder_state_dict=t(dec),
                                                                            postnet_state_dict=t(post)).to("cuda")
    return _cache["model"]


def clips_of(gu):
    return pc.oracle_clips(gu.la.synth)[:CLIPS]


def beams(gu, clips=None, caps=None, **kw):
    model = beam_model(gu)
    args = dict(num_beams=K_MODEL, num_return_sequences=K_MODEL, max_length=caps or CAPS, return_scores=True)
    args.update(kw)
    return model.beam_search_many(batches_of(gu, clips or clips_of(gu)), **args)


@pytest.fixture(scope="module")
def searched(gu):
    return beams(gu, return_step_logprobs=True)


def same_results(a, b, order=None):
    (ha, sa), (hb, sb) = a, b
    order = order or range(len(ha))
    for u, v in enumerate(order):
        assert len(ha[u]) == len(hb[v])
        for h in range(len(ha[u])):
            assert torch.equal(ha[u][h], hb[v][h]), (u, h)
            assert same_bits(sa[u][h].numpy(), sb[v][h].numpy())
        assert same_bits(ha.sequence_scores[u].numpy(), hb.sequence_scores[v].numpy())
        assert same_bits(ha.sequence_logprobs[u].numpy(), hb.sequence_logprobs[v].numpy())
    return True


def test_beam_search_many_replays_through_the_restatement(gu, searched):
    hyps, scores = searched
    V = beam_model(gu).speecht5.encoder._decoder_vocab
    lengths = set()
    for u in range(CLIPS):
        g = ref.BeamGroup(K_MODEL, V, max(CAPS), CAPS[u])
        for lp in hyps.step_logprobs[u].numpy():
            assert g.open and g.step(lp)
            g.reorder()
        assert not g.open
        want = g.finished()
        assert len(want) == len(hyps[u]) == K_MODEL
        for h, (tok, score, total, tlp) in enumerate(want):
            assert hyps[u][h].tolist() == tok, (u, h)
            assert float(hyps.sequence_scores[u][h]) == score and float(hyps.sequence_logprobs[u][h]) == total
            assert same_bits(scores[u][h].numpy(), tlp[1:])
            lengths.add(len(tok))
        assert sorted(hyps.sequence_scores[u].tolist(), reverse=True) == hyps.sequence_scores[u].tolist()
    assert len(lengths) >= 3, lengths  # not the trivial regime: hypotheses of several lengths
    assert all(len(hyps[u][h]) <= CAPS[u] for u in range(CLIPS) for h in range(K_MODEL))
    assert any(len(hyps[u][h]) == CAPS[u] for u in range(CLIPS) for h in range(K_MODEL))  # some ended in the step at their cap


def decode_beams(gu, items, slots, T_cap, S_max):
    """{key: (hypotheses, scores, sums, per-token log-probabilities)} of the items, in their order, through a fresh beam pool."""
    dec = importlib.import_module("loco-asr_amd.decoder")
    cfg = dec.check_beam_args(K_MODEL, K_MODEL)[2]
    pool = dec.DecoderPool(beam_model(gu).speecht5.encoder, slots, T_cap, S_max, torch.device("cuda", 0), beam=cfg)
    pool.submit(list(items))
    return {k: rest for k, *rest in pool.drain()}


def test_result_does_not_depend_on_slots_order_or_neighbours(gu, searched):
    """One encoder output (the packed encoder's sums depend on what is packed together, so the clips are encoded once, as the greedy
    pool's neighbour test does), decoded at slots = K, 2K and 64, in reversed admission order, and with and without a 30 s clip
    (T_enc = 1499 beside T_enc <= 149) in the pool: the same bits."""
    from test_gpu_decoder_pool import encode
    clips = clips_of(gu) + [(4, 480000)]
    items, out, _ = encode(gu, beam_model(gu), clips, CAPS + [5])
    T_cap, S_max = max(it.rows for it in items), max(CAPS)
    base = decode_beams(gu, items, 64, T_cap, S_max)
    assert sorted(base) == list(range(CLIPS + 1)) and all(len(base[k][0]) == K_MODEL for k in base)
    for slots, chosen in [(K_MODEL, items[:CLIPS]), (2 * K_MODEL, list(reversed(items))), (64, list(reversed(items[:CLIPS])))]:
        got = decode_beams(gu, chosen, slots, T_cap, S_max)
        assert sorted(got) == sorted(it.key for it in chosen)
        for k, (hyps, scores, sums, tlps, _) in got.items():
            want = base[k]
            assert len(hyps) == len(want[0])
            for h in range(len(hyps)):
                assert torch.equal(hyps[h], want[0][h]) and same_bits(tlps[h].numpy(), want[3][h].numpy()), (slots, k, h)
            assert same_bits(scores.numpy(), want[1].numpy()) and same_bits(sums.numpy(), want[2].numpy()), (slots, k)


def test_one_beam_is_greedy_and_greedy_is_untouched(gu, searched):
    model = beam_model(gu)
    batches = batches_of(gu, clips_of(gu))
    before, before_scores = model.generate_many(batches, max_length=CAPS, return_scores=True)
    one = model.beam_search_many(batches, num_beams=1, early_stopping=True, max_length=CAPS)
    for u in range(CLIPS):
        assert torch.equal(one[u][0], before[u]), u
    beams(gu)
    after, after_scores = model.generate_many(batches, max_length=CAPS, return_scores=True)
    for u in range(CLIPS):
        assert torch.equal(before[u], after[u]) and same_bits(before_scores[u].cpu().numpy(), after_scores[u].cpu().numpy())


# ---- 4. cache consistency ---------------------------------------------------------------------------------------------------------------
def forced_sums(model, batches, rows):
    """``model.score``'s sequence log-probability of one transcript per utterance (1-D ids from <s> on), batch by batch as the
    utterances were given: the labels are the ids after <s>, -100 behind a row's end."""
    out, u = [], 0
    for b in batches:
        mine = rows[u:u + int(b["input_values"].shape[0])]
        labels = torch.full((len(mine), max(int(r.shape[0]) for r in mine) - 1), -100, dtype=torch.long)
        for i, r in enumerate(mine):
            labels[i, :r.shape[0] - 1] = r[1:]
        out += model.score(b["input_values"], b["attention_mask"], labels=labels).sequence_logprob.double().cpu().tolist()
        u += len(mine)
    return out


def test_hypotheses_score_the_same_teacher_forced(gu, searched):
    """A hypothesis' sum of log-probabilities, collected step by step on a cache that was reordered after every step, against
    ``model.score``'s teacher-forced pass over the finished hypothesis.  The bar is 4 x the largest difference that greedy
    ``generate_many(return_scores=True)`` shows against ``model.score`` on the same clips in this run (4: another summation order);
    a wrong parent or a cache row that was not copied misses it by orders of magnitude."""
    model = beam_model(gu)
    hyps, _ = searched
    batches = batches_of(gu, clips_of(gu))
    ids, scores = model.generate_many(batches, max_length=CAPS, return_scores=True)
    greedy = [abs(float(s.double().sum()) - f) for s, f in zip(scores, forced_sums(model, batches, ids))]
    base = max(greedy)
    print("greedy |generate_many - score| per clip:", " ".join(f"{d:.3e}" for d in greedy), " lengths", [int(i.shape[0]) for i in ids])
    worst = 0.0
    for h in range(K_MODEL):
        forced = forced_sums(model, batches, [hyps[u][h] for u in range(CLIPS)])
        diffs = [abs(float(hyps.sequence_logprobs[u][h]) - forced[u]) for u in range(CLIPS)]
        print(f"beam {h} |beam - score| per clip:", " ".join(f"{d:.3e}" for d in diffs), " lengths", [int(hyps[u][h].shape[0]) for u in range(CLIPS)])
        worst = max(worst, max(diffs))
    print(f"beam vs teacher-forced: worst {worst:.3e}, greedy baseline {base:.3e}, bar {4 * base:.3e}")
    record_figure("decoder_beam_cache_consistency", worst=worst, greedy_baseline=base, bar=4 * base, hypotheses=CLIPS * K_MODEL)
    assert worst <= 4 * base, (worst, base)


# ---- 5. layout and command line -----------------------------------------------------------------------------------------------------------
def test_beam_search_layout(gu, searched):
    model = beam_model(gu)
    clips = clips_of(gu)[:2]
    x, m = pc.pairs(gu.la.synth, clips, 2)[0]
    out = model.beam_search(gu.dev(x), gu.dev(m, torch.int32), num_beams=K_MODEL, num_return_sequences=3, max_length=12)
    many, scores = beams(gu, clips=clips, caps=[12, 12], num_return_sequences=3)
    S = out.sequences.shape[1]
    assert out.sequences.shape == (6, S) and out.token_logprobs.shape == (6, S - 1) and out.sequences.is_cuda
    for b in range(2):
        for h in range(3):
            row, n = out.sequences[b * 3 + h].cpu(), many[b][h].shape[0]
            assert torch.equal(row[:n], many[b][h]) and bool((row[n:] == 1).all())
            assert same_bits(out.token_logprobs[b * 3 + h, :n - 1].cpu().numpy(), scores[b][h].numpy())
            assert bool((out.token_logprobs[b * 3 + h, n - 1:] == 0).all())
            assert float(out.sequences_scores[b * 3 + h]) == float(many.sequence_scores[b][h])
            assert float(out.sequence_logprobs[b * 3 + h]) == float(many.sequence_logprobs[b][h])
    with pytest.raises(NotImplementedError):
        model.generate(gu.dev(x), gu.dev(m, torch.int32), num_beams=4)
    with pytest.raises(ValueError, match="slots"):
        model.beam_search_many(batches_of(gu, clips), num_beams=4, slots=3)


def test_transcribe_long_takes_num_beams(gu, searched):
    """``num_beams=None`` is the greedy path; one beam with ``early_stopping=True`` gives its ids; four beams give the best beam of
    ``beam_search_many`` per segment, with that beam's scores."""
    from segment_cases import LONG, recording
    model = beam_model(gu)
    wave = gu.dev(recording())
    greedy = model.transcribe_long(wave, vad=LONG, max_length=12, return_scores=True)
    one = model.transcribe_long(wave, vad=LONG, max_length=12, return_scores=True, num_beams=1, early_stopping=True)
    four = model.transcribe_long(wave, vad=LONG, max_length=12, return_scores=True, num_beams=4, length_penalty=0.5)
    assert len(greedy.segments) == len(one.segments) == len(four.segments) >= 2
    for a, b, c in zip(greedy.segments, one.segments, four.segments):
        assert (a.start_s, a.end_s) == (b.start_s, b.end_s) == (c.start_s, c.end_s) and torch.equal(a.ids, b.ids)
        assert c.ids[0] == 2 and 2 <= c.ids.shape[0] <= 12 and c.token_logprobs.shape[0] == c.ids.shape[0] - 1
        assert c.logprob == float(c.token_logprobs.double().sum()) and c.avg_logprob == c.logprob / (c.ids.shape[0] - 1)
        clip = wave[round(c.start_s * 16000):round(c.end_s * 16000)][None]
        best = model.beam_search_many([dict(input_values=clip, attention_mask=torch.ones_like(clip, dtype=torch.int32))], num_beams=4,
                                      length_penalty=0.5, max_length=12)
        assert torch.equal(best[0][0], c.ids)
    with pytest.raises(ValueError, match="num_beams"):
        model.transcribe_long(wave, vad=LONG, num_beams=17)


def test_step_kinds_do_not_mix(gu, searched):
    """A beam pool refuses the greedy and sampling steps, a greedy pool the beam step: LOCO_E_STATE."""
    dec = importlib.import_module("loco-asr_amd.decoder")
    enc = beam_model(gu).speecht5.encoder
    _, _, cfg = dec.check_beam_args(2)
    dev = torch.device("cuda", 0)
    greedy = dec.DecoderPool(enc, 4, 8, 6, dev)
    lib, ws = enc._lib, greedy.workspace
    rc = lib.loco_decoder_pool_step_beam(enc._handle, 4, 8, 6, 0, 1, None, None, None, gu.ptr(ws), ws.numel(), gu.stream())
    assert rc == -2 and "beam" in lib.loco_last_error().decode()
    pool = dec.DecoderPool(enc, 4, 8, 6, dev, beam=cfg)
    out = torch.zeros((2, 8, 768), device="cuda")
    frames = torch.tensor([8, 8], dtype=torch.int32, device="cuda")
    pool.submit([dec.PoolItem(key=i, enc_out=out, frames=frames, clip=i, rows=8, cap=4) for i in range(2)])
    pool._fill()
    ws = pool.workspace
    assert lib.loco_decoder_pool_step(enc._handle, 4, 8, 6, 0, 8, None, gu.ptr(ws), ws.numel(), gu.stream()) == -2
    scfg = dec.check_sample_args(1, 1.0, 0, 1.0, 1)[1]
    assert lib.loco_decoder_pool_step_sample(enc._handle, 4, 8, 6, 0, 8, C.byref(scfg), None, None, gu.ptr(ws), ws.numel(), gu.stream()) == -2
    other = dec.check_beam_args(2, length_penalty=2.0)[2]
    one = (C.c_int32 * 1)(0)
    rc = lib.loco_decoder_pool_admit_beams(enc._handle, 4, 8, 6, C.byref(other), 1, one, gu.ptr(out), 8 * 768, one, None, one, gu.ptr(ws), ws.numel(),
                                           gu.stream())
    assert rc == -2
    assert len(pool.drain()) == 2  # and the pool still runs to its end


def test_command_line(gu, searched, tmp_path, monkeypatch):
    """``transcribe --beams``: the line's fields are the best beam, ``--nbest`` lists the N best with their scores, ``--select mbr``
    picks from that list; ``--beams 1 --early-stopping true`` writes the lines of the greedy pool."""
    tr = importlib.import_module("loco-asr_amd.transcribe")
    fe = importlib.import_module("loco-asr_amd.feature_extractor")
    model = beam_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)  # the CLI's own path from the arguments on
    common = ["--random-init", "--synthetic", "4", "--synthetic-seconds", "1.5", "--slots", "16", "--max-length", "12"]

    def run(extra):
        out = tmp_path / "out.jsonl"
        assert tr.main(common + extra + ["--out", str(out)]) == 0
        return out.read_text()

    items = tr.gather_items(tr.build_parser().parse_args(common))
    processor = fe.SpeechT5FeatureExtractorMI355X()
    feats = [tr.load_batch(items[b0:b0 + 2], b0, processor, torch.device("cuda", 0)) for b0 in (0, 2)]
    greedy = run([])
    assert run(["--beams", "1", "--early-stopping", "true"]) == greedy
    assert run(["--scores"]) != greedy
    want = model.beam_search_many(feats, num_beams=4, num_return_sequences=3, length_penalty=0.5, early_stopping="never", max_length=12, slots=16)
    flags = ["--beams", "4", "--length-penalty", "0.5", "--early-stopping", "never"]
    best = [json.loads(l) for l in run(flags).splitlines()]
    lines = [json.loads(l) for l in run(flags + ["--nbest", "3", "--scores"]).splitlines()]
    picked = [json.loads(l) for l in run(flags + ["--nbest", "3", "--select", "mbr"]).splitlines()]
    assert len(best) == len(lines) == len(picked) == 4
    for u, (b, l, m) in enumerate(zip(best, lines, picked)):
        n = len(want[u][0])
        assert set(b) == {"id", "token_ids"} and b["token_ids"][:n] == want[u][0].tolist() and all(t == 1 for t in b["token_ids"][n:])
        assert l["token_ids"] == b["token_ids"] and l["logprob"] == float(want.sequence_logprobs[u][0])
        assert abs(l["avg_logprob"] - l["logprob"] / (n - 1)) < 1e-12
        assert len(l["nbest"]) == 3
        for h, r in enumerate(l["nbest"]):
            assert list(r) == ["ids", "score", "logprob", "avg_logprob"]
            assert r["ids"] == want[u][h].tolist() and r["score"] == float(want.sequence_scores[u][h])
            assert r["logprob"] == float(want.sequence_logprobs[u][h]) and abs(r["avg_logprob"] - r["logprob"] / (len(r["ids"]) - 1)) < 1e-12
        assert [r["score"] for r in l["nbest"]] == sorted((r["score"] for r in l["nbest"]), reverse=True)
        risks = [r["mbr_risk"] for r in m["nbest"]]
        k = risks.index(min(risks))
        assert m["token_ids"][:len(m["nbest"][k]["ids"])] == m["nbest"][k]["ids"]
