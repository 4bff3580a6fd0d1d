"""The attention probabilities of output_attentions=True (attention_probs.hip) pinned per element, through both op entry points:

  f32        loco_op_attention_probs                       fp32 qkv, table given
  x3         loco_op_attention_probs_f16x3, terms 3        planes, table given
  x2         loco_op_attention_probs_f16x3, terms 2        planes, table given; the reference drops Q_hi K_lo as the kernel does
  x3_chain   loco_op_attention_probs_f16x3, terms 3        the table is the scratch a loco_op_attention_f16x3_pe launch with the same
                                                           frames has just filled, inside a NaN-sentinel allocation: what loco_forward does

Shapes are the smallest that take each path (32-key tiles, 32 query rows per wave, 128 per workgroup, |i - j| clipped at 160): T = 1, 31,
33, 64, 65, 129 (a second workgroup of one query), 161 (the first past-clipped key), 193, 225, 257, 449; B = 1-3; frames all valid, 1, 32,
33, T - 1.  Three cases -- (225, [1]), (257, [65, 64]), (449, [1, 64, 448]) -- have waves of padded queries for which the attention launch
forms NO table block (include/loco_asr.h, loco_op_attention_f16x3_pe): their scratch rows keep the sentinel, and the probabilities kernel
must not read them.  It does not: a row i >= n + 158, whose every valid key would read column 319, adds 0 instead.

Operands are those of tests/test_gpu_attention_contract.py (its Case, imported), placed the same hostile way (tests/op_check.py): q, k and
the table in NaN-filled allocations; of clip b with n valid keys the k rows [n, T) are NaN -- [32 ceil(n / 32), T) never read, [n, 32
ceil(n / 32)) read and discarded by a select; a table that is an input is NaN in every entry outside columns clip(i - n + 1) + 160 ...
clip(i) + 160 of row i, and in ALL of row i for i >= n + 158; P lives in a sentinel allocation: every P[b, h, i < T, j < T] is written
and nothing else.  Per launch: guards, masked keys the bits of +0.0f, a one-key clip exactly 1.0f in every row, everything finite, a
second run the same bits.  Per element: the fp64 softmax of the operands the kernel really multiplies (hi + lo of q and k) against the
bar derived in op_check's docstring, row sums against theirs, and P v in fp64 against the context of the attention kernels.
Scores of +-inf are outside the contract (the header says so); a key 30 or 80 nats above its row is inside it and tested here.
"""
import functools

import pytest
import torch

import test_gpu_attention_contract as tac
from conftest import record_figure

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import op_check as oc
    from gpu_util import check, lib, ptr, stream
    from op_check import Layout

F32 = torch.float32
HEADS, RELN, RELMAX = tac.HEADS, tac.RELN, tac.RELMAX
FORMS = ("f32", "x3", "x2", "x3_chain")
NO_READ = RELMAX - 2  # rows i >= n + 158 read no table entry

# (T, B, frames)
CASES = [(1, 1, None), (31, 2, [1, 30]), (33, 3, [32, 33, 1]), (64, 1, None), (65, 3, [64, 33, 32]), (129, 2, [129, 128]), (161, 2, [161, 1]),
         (193, 1, [33]), (225, 1, [1]), (225, 3, None), (257, 2, [65, 64]), (449, 3, [1, 64, 448]), (449, 3, [0, 450, -3])]
HAZARD = [(225, 1, [1]), (257, 2, [65, 64]), (449, 3, [1, 64, 448])]
# head h of the massive-activation case: key js scores D nats above its row.  n = 150: tile 0 (r = 5, 21), a later tile (r = 6, 26) and the
# last, partial tile 128 ... 149 (r = 3, 20): both ends of the butterfly's 16-lane step, each at 30 and at 80 nats
MASSIVE = (161, 1, [150])
OUTLIERS = [(js, D) for D in (30.0, 80.0) for js in (5, 21, 70, 90, 131, 148)]


def case_id(ci):
    T, B, frames = CASES[ci]
    return f"T{T}-B{B}-" + ("all" if frames is None else ".".join(str(f) for f in frames))


@functools.lru_cache(maxsize=None)
def case(ci):
    """the operands: the attention contract's own Case where it has the shape, else one built the same way"""
    key = CASES[ci] + (False,)
    return tac.case(tac.CASES.index(key)) if key in tac.CASES else tac.Case(key)


class Massive(tac.Case):
    def __init__(self):
        super().__init__(MASSIVE + (False,))
        i = torch.arange(self.T)
        for h, (js, D) in enumerate(OUTLIERS):
            assert int((i - js).abs().max()) < RELMAX - 1  # a column of its own in every row
            self.tab32[0, h, i, i - js + RELMAX] += D
        self.tab64 = self.ref = None  # the table is an input here; nothing of the attention references applies


@functools.lru_cache(maxsize=None)
def massive():
    return Massive()


@functools.lru_cache(maxsize=3)
def reference(c, form):
    """fp64 P of `form` on Case c and its bars (op_check.probs_bar): dict P, rel, row_sum_bar, n"""
    T, B = c.T, c.B
    q = c.q64
    k = tac.heads(c.kh.double()) if form == "x2" else c.k64
    i, j = torch.arange(T)[:, None], torch.arange(T)[None]
    idx = ((i - j).clamp(-RELMAX, RELMAX - 1) + RELMAX).expand(B, HEADS, T, T)
    n = torch.tensor(c.n).view(B, 1, 1, 1)
    valid = j[None, None] < n
    reads = (i[None, None] < n + NO_READ).expand(B, HEADS, T, T)
    chain = form == "x3_chain"
    bias = (c.tab64 if chain else c.tab32.double()).gather(-1, idx).masked_fill(~reads, 0.0)
    table_abs = c.tab_abs.gather(-1, idx).masked_fill(~reads, 0.0) if chain else None
    s = q @ k.transpose(-1, -2)
    A = q.abs() @ k.abs().transpose(-1, -2)
    P = torch.softmax((s + bias).masked_fill(~valid, float("-inf")), -1)
    _, rel, row_sum_bar = oc.probs_bar("x3" if chain else form, P, s, bias, A, valid, n.double(), table_abs)
    return dict(P=P, rel=rel, row_sum_bar=row_sum_bar, n=n)


@functools.lru_cache(maxsize=None)
def probs_table(c, clip):
    """the given table of c.placed(clip=clip), with every entry of the rows that read none (i >= n + 158) NaN as well"""
    d = c.placed(clip=clip)
    tab = oc.owned(d["tab"], d["lt"]).view(d["B"], HEADS, c.T, RELN).clone()
    for b, nb in enumerate(d["n"]):
        tab[b, :, nb + NO_READ:] = float("nan")
    return oc.poisoned(tab.view(1, 1, -1, RELN), d["lt"])


def launch(form, c, clip=None, frames="own"):
    """One launch of `form` on the placed operands of Case c into a fresh sentinel-filled P; the guards are asserted here, for every
    launch of this file.  -> P [B, 12, T, T]"""
    T = c.T
    d = c.placed(clip=clip)
    B, lp = d["B"], d["lp"]
    lP = Layout(B * HEADS * T, T)
    P = oc.sentinel_buffer(lP, F32)
    fr = ptr(d["frames"] if frames == "own" else frames)
    q_k = [oc.base(d[name], lp) for name in ("qh", "ql", "kh", "kl")]
    if form == "x3_chain":
        if frames != "own":
            d = dict(d, frames=frames)
        scratch = tac.launch("x3_pe", d, T)["scratch"]  # sentinel-filled, guards asserted: only the formed entries are written
        qp = oc.base(scratch, d["scratch_layout"])
    else:
        qp = oc.base(probs_table(c, clip), d["lt"])
    if form == "f32":
        check(lib().loco_op_attention_probs(oc.base(d["qkv"], d["lq"]), qp, fr, oc.base(P, lP), B, T, stream()), form)
    else:
        check(lib().loco_op_attention_probs_f16x3(*q_k, qp, fr, oc.base(P, lP), B, T, 2 if form == "x2" else 3, stream()), form)
    torch.cuda.synchronize()
    oc.assert_guards(P, lP, f"{form} P")
    return oc.owned(P, lP).view(B, HEADS, T, T)


def assert_structure(P, n, what):
    """masked keys the bits of +0.0f; a one-key clip exactly 1.0f in every row, padded rows included; every element finite"""
    assert bool(torch.isfinite(P).all()), f"{what}: {int((~torch.isfinite(P)).sum())} non-finite probabilities, first at " \
                                          f"{torch.nonzero(~torch.isfinite(P))[0].tolist()}"
    for b, nb in enumerate(n):
        masked = P[b, :, :, nb:].contiguous().view(torch.int32)
        assert not bool((masked != 0).any()), f"{what}: clip {b}: {int((masked != 0).sum())} masked keys are not +0.0f"
        if nb == 1:
            assert bool((P[b, :, :, 0] == 1.0).all()), f"{what}: clip {b}: a one-key row is not exactly 1"


def assert_elements(P, r, **tags):
    """every element within its bar, every row sum within its own; the measured maxima are recorded"""
    got = P.double().cpu()
    err = (got - r["P"]).abs()
    bar = r["P"] * r["rel"] + oc.FLT_MIN
    worst = float((err / bar).max())
    big = r["P"] >= 2.0 ** -100  # err / (u P) means nothing beside a flush; below, the bar is its FLT_MIN and a flushed result may use all of it
    ratio = float((err[big] / (oc.U * r["P"][big])).max())
    worst_big = float((err[big] / bar[big]).max())
    rs = (got.sum(-1, keepdim=True) - 1).abs()
    rs_worst = float((rs / r["row_sum_bar"]).max())
    record_figure("attention_probs_contract", max_err_over_bar=round(worst, 4), max_err_over_bar_above_2_100=round(worst_big, 4),
                  max_err_over_uP=round(ratio, 3),
                  max_row_sum_dev=float(f"{float(rs.max()):.3e}"), max_row_sum_dev_over_bar=round(rs_worst, 4), **tags)
    print(f"attention_probs_contract {tags}: max err / bar = {worst:.4f} ({worst_big:.4f} over P >= 2^-100), max err / (u P) = {ratio:.3f}, max |row sum - 1| = "
          f"{float(rs.max()):.3e} ({rs_worst:.4f} of its bar)")
    if worst > 1.0:
        at = torch.nonzero(err / bar == (err / bar).max())[0].tolist()
        raise AssertionError(f"{tags}: P{at} is {worst:.3g} x its bar (err {float(err[tuple(at)]):.3e}, P {float(r['P'][tuple(at)]):.3e}); "
                             f"{int((err > bar).sum())} elements over")
    assert rs_worst <= 1.0, f"{tags}: a row sum is {rs_worst:.3g} x its bar off 1"


ALL = [(ci, form) for ci in range(len(CASES)) for form in FORMS]
ids = lambda pairs: [f"{case_id(ci)}-{form}" for ci, form in pairs]


@pytest.mark.parametrize("ci,form", ALL, ids=ids(ALL))
def test_guards_structure_same_bits_and_every_element(ci, form):
    c = case(ci)
    P = launch(form, c)
    assert_structure(P, c.n, f"{case_id(ci)} {form}")
    assert oc.same_bits(P, launch(form, c)), "a second run gives other bits"
    assert_elements(P, reference(c, form), form=form, case=case_id(ci))


BATCHED = [(ci, form) for ci in range(len(CASES)) for form in FORMS if CASES[ci][1] == 3]


@pytest.mark.parametrize("ci,form", BATCHED, ids=ids(BATCHED))
def test_clip_of_a_batch_equals_its_own_launch(ci, form):
    c = case(ci)
    full = launch(form, c)
    for b in range(3):
        assert oc.same_bits(full[b:b + 1].contiguous(), launch(form, c, clip=b)), f"clip {b} differs from its B = 1 launch"


@pytest.mark.parametrize("form", FORMS)
def test_out_of_range_frames_mean_every_key(form):
    """frames <= 0 and > T are T: [0, 450, -3] at T = 449 against frames = NULL"""
    c = case(CASES.index((449, 3, [0, 450, -3])))
    assert oc.same_bits(launch(form, c), launch(form, c, frames=None)), "frames [0, 450, -3] against NULL"


@pytest.mark.parametrize("form", FORMS)
def test_unformed_scratch_rows_are_not_read(form):
    """The hazard, stated by itself: the probabilities of a padded query row i >= n + 158 are those of its scores alone -- finite whatever
    the table holds there (a NaN input row; the untouched sentinel of the attention launch's scratch), and rows from 224 on of a clip of at
    most 64 frames are exactly such rows."""
    for T, B, frames in HAZARD:
        c = case(CASES.index((T, B, frames)))
        P = launch(form, c)
        for b, nb in enumerate(c.n):
            if nb <= 64 and T > 224:
                if form == "x3_chain":
                    assert not bool(tac.formed_columns(T, nb)[224:].any())  # the launch forms nothing there
                rows = P[b, :, 224:]
                assert bool(torch.isfinite(rows).all()), f"T {T} frames {frames} clip {b}: rows from 224 on are not finite"


CROSS = [(ci, form) for ci in (CASES.index((65, 3, [64, 33, 32])), CASES.index((257, 2, [65, 64])), CASES.index((449, 3, [1, 64, 448])))
         for form in ("f32", "x3")]


@pytest.mark.parametrize("ci,form", CROSS, ids=ids(CROSS))
def test_probabilities_are_those_the_context_was_made_from(ci, form):
    """P v in fp64 against the context loco_op_attention / loco_op_attention_f16x3 return for the same placed inputs, within the sum of
    the two derived bars (op_check, part 5 of the probabilities bar and the attention bar)"""
    c = case(ci)
    r = reference(c, form)
    ctx = tac.heads(tac.launch(form, c.placed(), c.T)["ctx"].double().cpu())
    Pv = launch(form, c).double().cpu() @ c.v64
    ra, attn_bar = c.bar(form)
    bar = attn_bar + r["rel"] * ra["S"] + r["n"].double() * oc.FLT_MIN * c.v64.abs().amax()
    oc.assert_elements("attention_probs_contract_context", Pv, ctx, ra["S"], bar, form=form, case=case_id(ci))


@pytest.mark.parametrize("form", FORMS[:3])
def test_massive_activation_rows(form):
    """head h: key OUTLIERS[h][0] outscores the rest of every row by OUTLIERS[h][1] nats (30 or 80), in tile 0, a later tile and the last,
    partial tile, at r < 16 and r >= 16: finite, and within the same bar"""
    c = massive()
    P = launch(form, c)
    assert_structure(P, c.n, f"massive {form}")
    r = reference(c, form)
    for h, (js, D) in enumerate(OUTLIERS):
        others = torch.cat([r["P"][0, h, :, :js], r["P"][0, h, :, js + 1:]], -1)
        assert float(others.max()) < float(torch.exp(torch.tensor(15.0 - D))), "the placed key does not dominate its rows"  # the inputs' own check
    assert_elements(P, r, form=form, case="massive-T161-150")
