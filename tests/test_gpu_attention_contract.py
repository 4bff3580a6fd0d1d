"""Encoder attention (attention_f32.hip, attention_f16x3.hip) pinned per element, through every op entry point:

  f32        loco_op_attention                              fp32 qkv, table given
  x3         loco_op_attention_f16x3                        planes, table given, fp32 context
  x3_pe      loco_op_attention_f16x3_pe                     planes, the kernel forms the table, fp32 context
  planes     loco_op_attention_f16x3_planes (pe NULL)       planes, table given, context as hi/lo planes
  planes_pe  loco_op_attention_f16x3_planes (pe planes)     the instantiation loco_forward launches

Shapes are the smallest that take each path of the kernels (64-key tiles, 32 queries per wave, 128 per workgroup, |i - j| clipped at 160):
T = 1 (waves 1-3 hold no query), 33 (a wave with one query, a partial tile), 64 (one full tile), 65 (a second tile of one key), 129 (a
second query block of one query), 193 (first future-clipped tile: wave 0, tile 192), 225 (first past-clipped tile: one query), 257 (five
tiles), 449 (four query blocks, both clips); B = 1, 2, 3 puts 12 B nqb at 0 and at 4 mod 8 in the XCD work map.

Every launch here runs on hostile inputs and guarded outputs (tests/op_check.py):
  * q, k, v and the table sit in NaN-filled allocations; of clip b with n = frames[b] valid keys and R = min(T, 64 ceil(n / 64)), the k and
    v rows [R, T) are NaN (never read), the k rows [n, R) are NaN (read, masked by a select), and the v rows [n, R) hold finite data (read
    and multiplied by a probability of exactly zero: the contract of include/loco_asr.h);
  * a table that is an input is NaN in every entry that no valid key reads.  That set is clean: the valid keys j < n of query i read the
    columns clip(i - n + 1) + 160 ... clip(i) + 160, and the constants of clipped tiles (columns 0 and 319) always lie inside it -- a
    past-clipped tile means i0 >= 222, so key 0 reads column 319; a future-clipped tile starts at a valid key j0 >= i + 160, which reads
    column 0 (readable_columns() asserts both);
  * outputs -- ctx, ctx_hi, ctx_lo and the table scratch of the pe forms -- are sentinel-filled; the scratch's owned set is exactly what
    the header's formula says is formed, everything else must keep the sentinel's bits.
The fp64 reference is taken on the operands the kernel really multiplies (hi + lo of q, k, v and pe; the fp32 kernel gets exactly those sums,
which fp32 holds exactly), per element against the bar derived in op_check's docstring, with the whole-tensor bars of tests/test_gpu_ops.py
(3e-6 fp32, 1e-5 f16x3) kept beside it.

The "coherent" case (T = 257) gives ONE of the three MFMA terms of the score product its full weight: with random planes the
K_lo Q_hi^T contributions of different keys and channels partly cancel in the output (a kernel without the term still misses the bar of
the random cases, by 3 to 9 times).  There q has one sign pattern per channel for every query, the k_lo planes follow that pattern for even
keys and oppose it for odd keys, and v is +-|v| by key parity: K_lo Q_hi^T then moves every even key's score up and every odd key's down
by about 2^-13 sum |q| |k|, and the output by about that times S -- 18 to 25 times the bar if the term is missing.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import op_check as oc
    from gpu_util import check, la, lib, ptr, stream
    from op_check import Layout, Subset, knobs

F16, F32 = torch.float16, torch.float32
HEADS, HD, HID, RELN, RELMAX = 12, 64, 768, 320, 160
FORMS = ("f32", "x3", "x3_pe", "planes", "planes_pe")

# (T, B, frames, coherent)
CASES = [(1, 1, None, False), (33, 2, None, False), (64, 1, None, False), (65, 3, None, False), (129, 2, None, False), (193, 1, None, False),
         (193, 2, [193, 192], False), (225, 3, None, False), (257, 1, None, False), (257, 2, [257, 129], False), (257, 2, [65, 64], False),
         (257, 1, None, True), (449, 1, None, False), (449, 3, [449, 191, 65], False), (449, 3, [1, 64, 448], False),
         (449, 3, [0, 450, -3], False)]


def case_id(ci):
    T, B, frames, coherent = CASES[ci]
    return f"T{T}-B{B}-" + ("all" if frames is None else ".".join(str(f) for f in frames)) + ("-coherent" if coherent else "")


def find_case(T, B, frames):
    return CASES.index((T, B, frames, False))


def valid_keys(T, B, frames):
    """the kernels' rule: frames NULL, <= 0 or > T mean T"""
    return [T if frames is None or frames[b] <= 0 or frames[b] > T else frames[b] for b in range(B)]


def hu(key, shape, scale=1.0):
    return torch.from_numpy(la.synth.hashed_uniform(key, shape, 11)) * scale


def host_planes(x):
    hi = x.half()
    return hi, (x - hi.float()).half()


def heads(x):
    """[B, T, 768] -> [B, 12, T, 64]"""
    return x.view(x.shape[0], x.shape[1], HEADS, HD).transpose(1, 2)


def readable_columns(T, n):
    """bool [T, 320]: the table entries of one clip that a valid key or a clipped tile's constant reads (module docstring)"""
    i = torch.arange(T)[:, None]
    c = torch.arange(RELN)[None]
    by_key = (c >= (i - n + 1).clamp(-RELMAX, RELMAX - 1) + RELMAX) & (c <= i.clamp(max=RELMAX - 1) + RELMAX)
    i0 = 32 * (i // 32)
    ntiles = (n + 63) // 64
    past = i0 - 63 >= RELMAX - 1                            # tile 0 is past-clipped for this wave
    future = i0 + 31 - 64 * (ntiles - 1) <= -RELMAX         # the last tile is future-clipped
    const = (past & (c == RELN - 1)) | (future & (c == 0))
    assert not bool((const & ~by_key).any())
    return by_key | const


def formed_columns(T, n):
    """bool [T, 320]: what include/loco_asr.h says a pe-form launch leaves in row i of qp_scratch"""
    i0 = 32 * (torch.arange(T)[:, None] // 32)
    nk = 64 * ((n + 63) // 64)
    lo = (i0 - (nk - 1)).clamp(min=-RELMAX)
    hi = (i0 + 31).clamp(max=RELMAX - 1)
    c = torch.arange(RELN)[None]
    return (c >= 32 * ((lo + RELMAX) // 32)) & (c <= 32 * ((hi + RELMAX) // 32) + 31)


class Case:
    """Operands of one (T, B, frames) on the host as fp16 planes, the fp64 references of both table forms, and the hostile device
    placements.  Built once per case and shared by every test of that case; nothing in it is modified afterwards."""

    def __init__(self, ci):
        T, B, frames, coherent = CASES[ci] if isinstance(ci, int) else ci  # an index into CASES, or a (T, B, frames, coherent) of the caller's
        self.T, self.B, self.frames = T, B, frames
        self.n = valid_keys(T, B, frames)
        qkv = hu("atc.qkv", (B, T, 2304), 1.5)
        qkv[..., :HID] *= 0.125 * 1.5  # q arrives pre-scaled
        pe_k = hu("atc.pe", (RELN, HD), 0.9)
        q, k, v = qkv[..., :HID].clone(), qkv[..., HID:2 * HID].clone(), qkv[..., 2 * HID:].clone()
        if coherent:
            sign_c = torch.where(hu("atc.sign", (HID,)) < 0, -1.0, 1.0)
            parity = torch.where(torch.arange(T) % 2 == 0, 1.0, -1.0)[None, :, None]
            q = q.abs() * sign_c
            v = v.abs() * parity
        self.qh, self.ql = host_planes(q)
        self.kh, self.kl = host_planes(k)
        self.vh, self.vl = host_planes(v)
        if coherent:  # |lo| in [1/4, 3/4) 2^-12 |hi|: a legitimate low plane (hi + lo still fits fp32), its sign chosen per key and channel
            mag = self.kh.float().abs() * 2.0 ** -12 * (0.5 + 0.25 * hu("atc.lo", (B, T, HID)))
            kl = (mag * sign_c * parity).half()
            self.kl = ((self.kh.float() + kl.float()) - self.kh.float()).half()  # on fp32's grid, so that hi + lo is an fp32 number
        self.ph, self.pl = host_planes(pe_k * 512.0)
        f64 = lambda hi, lo: hi.double() + lo.double()
        self.q64, self.k64, self.v64 = heads(f64(self.qh, self.ql)), heads(f64(self.kh, self.kl)), heads(f64(self.vh, self.vl))
        self.pe64 = f64(self.ph, self.pl) / 512.0
        for x in (self.q64, self.k64, self.v64):
            assert bool((x.float().double() == x).all())  # the fp32 kernel's operands are exactly these sums
        self._reference()
        self._placed = {}

    def _reference(self):
        T, B = self.T, self.B
        q, k, v = self.q64, self.k64, self.v64
        i, j = torch.arange(T)[:, None], torch.arange(T)[None]
        idx = ((i - j).clamp(-RELMAX, RELMAX - 1) + RELMAX).expand(B, HEADS, T, T)
        valid = (j[None, None] < torch.tensor(self.n)[:, None, None, None])  # [B, 1, 1, T]
        s = q @ k.transpose(-1, -2)
        rowmax = lambda x: x.masked_fill(~valid, 0.0).amax(-1, keepdim=True)
        A_max, s_max = rowmax(q.abs() @ k.abs().transpose(-1, -2)), rowmax(s.abs())
        self.tab64 = q @ self.pe64.t()                      # [B, 12, T, 320]
        self.tab_abs = q.abs() @ self.pe64.abs().t()
        self.tab32 = self.tab64.float()                     # the table as an INPUT: an operand, rounded once on the host
        P_max = rowmax(self.tab_abs.gather(-1, idx))
        self.ntiles = ((torch.tensor(self.n) + 63) // 64).double().view(B, 1, 1, 1)
        self.ref = {}
        for table, tab in (("given", self.tab32.double()), ("formed", self.tab64)):
            bias = tab.gather(-1, idx)
            w = torch.softmax((s + bias).masked_fill(~valid, float("-inf")), -1)
            self.ref[table] = dict(ref=w @ v, S=w @ v.abs(), A_max=A_max, P_max=P_max, s_max=s_max, b_max=rowmax(bias.abs()))

    def bar(self, form):
        r = self.ref["formed" if form.endswith("_pe") else "given"]
        return r, oc.attention_bar("f32" if form == "f32" else "f16x3", r["ref"], r["S"], r["A_max"], r["P_max"], r["s_max"], r["b_max"],
                                   self.ntiles, form.endswith("_pe"), form.startswith("planes"))

    def placed(self, vfill=None, clip=None):
        """The device inputs.  vfill: what the v rows [n, R) hold -- None: the random data, "zero", "big": +-65504 in both planes (+-3e38
        for the fp32 kernel).  clip = b: that clip alone, as a B = 1 problem."""
        key = (vfill, clip)
        if key not in self._placed:
            self._placed[key] = self._place(vfill, clip)
        return self._placed[key]

    def _place(self, vfill, clip):
        T = self.T
        sel = slice(None) if clip is None else slice(clip, clip + 1)
        n = self.n if clip is None else [self.n[clip]]
        B = len(n)
        t = {name: getattr(self, name)[sel].clone() for name in ("qh", "ql", "kh", "kl", "vh", "vl")}
        v32 = t["vh"].float() + t["vl"].float()
        nan = float("nan")
        for b in range(B):
            R = min(T, 64 * ((n[b] + 63) // 64))
            for name in ("kh", "kl"):
                t[name][b, n[b]:] = nan
            for name in ("vh", "vl"):
                t[name][b, R:] = nan
            v32[b, R:] = nan
            if vfill is not None and R > n[b]:
                sign = torch.where((torch.arange(n[b], R)[:, None] + torch.arange(HID)[None]) % 2 == 0, 1.0, -1.0)
                for name in ("vh", "vl"):
                    t[name][b, n[b]:R] = (65504.0 * sign).half() if vfill == "big" else 0.0
                v32[b, n[b]:R] = 3e38 * sign if vfill == "big" else 0.0
        qkv32 = torch.cat([t["qh"].float() + t["ql"].float(), t["kh"].float() + t["kl"].float(), v32], -1)
        tab = self.tab32[sel].clone()
        for b in range(B):
            tab[b, :, ~readable_columns(T, n[b])] = nan
        lp, lq, lt, lpe = Layout(B * T, HID), Layout(B * T, 3 * HID), Layout(B * HEADS * T, RELN), Layout(RELN, HD)
        d = {name: oc.poisoned(x.cuda().view(1, 1, B * T, HID), lp) for name, x in t.items()}
        d.update(B=B, n=n, lp=lp, lq=lq, lt=lt, lpe=lpe, qkv=oc.poisoned(qkv32.cuda().view(1, 1, B * T, 3 * HID), lq),
                 tab=oc.poisoned(tab.cuda().view(1, 1, B * HEADS * T, RELN), lt),
                 ph=oc.poisoned(self.ph.cuda().view(1, 1, RELN, HD), lpe), pl=oc.poisoned(self.pl.cuda().view(1, 1, RELN, HD), lpe))
        formed = torch.stack([formed_columns(T, nb) for nb in n])[:, None].expand(B, HEADS, T, RELN)
        d["formed"] = formed
        d["scratch_layout"] = Subset(torch.nonzero(formed.reshape(-1)).reshape(-1), B * HEADS * T * RELN)
        d["frames"] = None if self.frames is None else torch.tensor(self.frames[sel], dtype=torch.int32).cuda()
        return d


@functools.lru_cache(maxsize=None)
def case(ci):
    return Case(ci)


def launch(form, d, T):
    """One launch of `form` on the placed inputs d into fresh sentinel-filled outputs; the guards are asserted here, for every launch of
    this file.  Returns the outputs: "ctx" [B, T, 768] fp32, or "hi" / "lo"; and "scratch", the whole guarded allocation of the pe forms."""
    B, lp, lc = d["B"], d["lp"], Layout(d["B"] * T, HID)
    planes_in = [oc.base(d[name], lp) for name in ("qh", "ql", "kh", "kl", "vh", "vl")]
    pe = form.endswith("_pe")
    out = {}
    if pe:
        out["scratch"] = oc.sentinel_buffer(d["scratch_layout"], F32)
        qp = oc.base(out["scratch"], d["scratch_layout"])
    else:
        qp = oc.base(d["tab"], d["lt"])
    if form.startswith("planes"):
        out["hi"], out["lo"] = oc.sentinel_buffer(lc, F16), oc.sentinel_buffer(lc, F16)
    else:
        out["ctx"] = oc.sentinel_buffer(lc, F32)
    fr = ptr(d["frames"])
    if form == "f32":
        check(lib().loco_op_attention(oc.base(d["qkv"], d["lq"]), qp, fr, oc.base(out["ctx"], lc), B, T, stream()), form)
    elif form == "x3":
        check(lib().loco_op_attention_f16x3(*planes_in, qp, fr, oc.base(out["ctx"], lc), B, T, stream()), form)
    elif form == "x3_pe":
        check(lib().loco_op_attention_f16x3_pe(*planes_in, oc.base(d["ph"], d["lpe"]), oc.base(d["pl"], d["lpe"]), 1.0 / 512.0, qp, fr,
                                               oc.base(out["ctx"], lc), B, T, stream()), form)
    else:
        pes = (oc.base(d["ph"], d["lpe"]), oc.base(d["pl"], d["lpe"])) if pe else (None, None)
        check(lib().loco_op_attention_f16x3_planes(*planes_in, *pes, 1.0 / 512.0, qp, fr, oc.base(out["hi"], lc), oc.base(out["lo"], lc),
                                                   B, T, stream()), form)
    torch.cuda.synchronize()
    for name, buf in out.items():
        oc.assert_guards(buf, d["scratch_layout"] if name == "scratch" else lc, f"{form} {name}")
    for name in ("ctx", "hi", "lo"):
        if name in out:
            out[name] = oc.owned(out[name], lc).view(B, T, HID)
    return out


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        bits = torch.int16 if a[name].dtype == F16 else torch.int32
        diff = a[name].contiguous().view(bits) != b[name].contiguous().view(bits)
        assert not bool(diff.any()), f"{what}: {name} differs in {int(diff.sum())} elements, first at {torch.nonzero(diff)[0].tolist()}"


ALL = [(ci, form) for ci in range(len(CASES)) for form in FORMS]
ids = lambda pairs: [f"{case_id(ci)}-{form}" for ci, form in pairs]


@pytest.mark.parametrize("ci,form", ALL, ids=ids(ALL))
def test_guards_poisoned_inputs_and_every_element(ci, form):
    """(a) guards, (b) poisoned inputs, (f) every element against its derived bar -- and the entries of the table the pe forms leave"""
    c = case(ci)
    T, B = c.T, c.B
    d = c.placed()
    out = launch(form, d, T)
    got = out["ctx"].double() if "ctx" in out else out["hi"].double() + out["lo"].double()
    r, bar = c.bar(form)
    oc.assert_elements("attention_contract", heads(got.cpu()), r["ref"], r["S"], bar, rel_l2_bar=3e-6 if form == "f32" else 1e-5,
                       form=form, case=case_id(ci))
    if form.endswith("_pe"):
        formed = d["formed"].reshape(-1)
        table = oc.owned(out["scratch"], d["scratch_layout"]).reshape(-1)
        want, scale = c.tab64.reshape(-1)[formed], c.tab_abs.reshape(-1)[formed]
        oc.assert_elements("attention_contract_table", table, want, scale, (oc.f16x3_count(64) + 1) * oc.U * scale, form=form, case=case_id(ci))


MASKED = [(ci, form) for ci in range(len(CASES)) for form in FORMS
          if any(n % 64 and n < CASES[ci][0] for n in valid_keys(*CASES[ci][:3]))]


@pytest.mark.parametrize("ci,form", MASKED, ids=ids(MASKED))
def test_masked_v_rows_change_no_bit(ci, form):
    """(c) v rows [n, R) are read and multiplied by a probability of exactly zero: +-65504 in both planes (+-3e38 in fp32) there
    gives the bits that zeros give"""
    c = case(ci)
    assert_same_bits(launch(form, c.placed("big"), c.T), launch(form, c.placed("zero"), c.T), "huge against zero masked v rows")


BOTH_TABLES = [(ci, pe) for ci in range(len(CASES)) for pe in ("", "_pe")]


@pytest.mark.parametrize("ci,pe", BOTH_TABLES, ids=[f"{case_id(ci)}-{'formed' if pe else 'given'}" for ci, pe in BOTH_TABLES])
def test_plane_outputs_are_the_split_of_the_fp32_context(ci, pe):
    """(d) ctx_hi / ctx_lo of the planes entry against loco_op_split_f16 of the fp32 context of the same operands and table form"""
    c = case(ci)
    d = c.placed()
    ctx = launch("x3" + pe, d, c.T)["ctx"]
    out = launch("planes" + pe, d, c.T)
    hi, lo = oc.split_planes(ctx)
    torch.cuda.synchronize()
    for name, want in (("hi", hi), ("lo", lo)):
        diff = out[name].view(torch.int16) != want.view(torch.int16)
        assert not bool(diff.any()), f"ctx_{name}: {int(diff.sum())} elements differ, first at {torch.nonzero(diff)[0].tolist()}"


BATCHED = [(ci, form) for ci in range(len(CASES)) for form in FORMS if CASES[ci][1] == 3]


@pytest.mark.parametrize("ci,form", BATCHED, ids=ids(BATCHED))
def test_clip_of_a_batch_equals_its_own_launch(ci, form):
    """(e) the work map: clip b of a B = 3 launch against a B = 1 launch of that clip alone, bit for bit (table scratch included)"""
    c = case(ci)
    T = c.T
    full = launch(form, c.placed(), T)
    per = HEADS * T * RELN
    for b in range(3):
        one = launch(form, c.placed(clip=b), T)
        for name in one:
            if name == "scratch":
                head = c.placed()["scratch_layout"].head
                assert oc.same_bits(full[name][head + b * per:head + (b + 1) * per], one[name][head:head + per]), f"clip {b}: scratch differs"
            else:
                assert oc.same_bits(full[name][b:b + 1], one[name]), f"clip {b}: {name} differs"


@pytest.mark.parametrize("form", FORMS)
def test_out_of_range_frames_mean_every_key(form):
    """(e) frames <= 0 and > T are T in both kernels: [0, 450, -3] at T = 449 against frames = NULL"""
    c = case(find_case(449, 3, [0, 450, -3]))
    d = dict(c.placed())
    d["frames"] = None
    assert_same_bits(launch(form, c.placed(), 449), launch(form, d, 449), "frames [0, 450, -3] against NULL")


LONG = [(find_case(65, 3, None), f) for f in FORMS[1:]] + [(find_case(225, 3, None), f) for f in FORMS[1:]] + \
       [(find_case(449, 3, [449, 191, 65]), f) for f in FORMS[1:]]


@pytest.mark.parametrize("ci,form", LONG, ids=ids(LONG))
def test_long_sequence_instantiation_gives_the_same_bits(ci, form):
    """(e) LOCO_ATTN_LONG = 1 (the rescale skipped where alpha == 1 in every lane) against 0, all four f16x3 instantiation pairs"""
    c = case(ci)
    with knobs(LOCO_ATTN_LONG="1"):
        long_ = launch(form, c.placed(), c.T)
    with knobs(LOCO_ATTN_LONG="0"):
        short = launch(form, c.placed(), c.T)
    assert_same_bits(long_, short, "LOCO_ATTN_LONG 1 against 0")
