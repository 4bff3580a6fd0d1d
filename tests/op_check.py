"""Per-element checks of single operators: guarded outputs, poisoned inputs, fp64 references and derived error bars.

Used by tests/test_gpu_gemm_contract.py, tests/test_gpu_attention_contract.py, tests/test_gpu_attention_probs_contract.py,
tests/test_gpu_decoder_contract.py, tests/test_gpu_frontend_contract.py and (on the CPU) tests/test_decoder_contract_ref.py and
tests/test_frontend_ref.py.  Nothing here is fitted to a kernel's output: every bar below is a worst-case count of
roundings times the forward-error scale of the element it applies to.

Guards.  An output lives inside a larger allocation filled with a sentinel bit pattern (a NaN with a payload): before the first
owned element, after the last (at least one 256 x 256 tile of rows), in the ld - N pad of every row and in the gaps between
batch entries.  After a launch every element the operator does not own must still hold the sentinel's bits, and no owned element
may (a NaN with that payload is not something the arithmetic produces).  Inputs are laid out the same way with NaN everywhere the
kernel has no business reading a VALUE from: pads, gaps, rows past the end.  (The kernels clamp row indices to the last row and
read only k in [0, K); a NaN that reaches an accumulator shows in the output.)

Error bars, u = 2^-24, S[m,n] = sum_k |a_k| |w_k| + |bias[n]| + |R[m,n]| (with out_scale folded into the sum).
  f16x3 (gemm_f16x3.hip): an element is accumulated k-tile by k-tile (32 deep), `terms` MFMAs per k-tile, each charged two
    roundings of at most u * |partial sum| <= u S; plus 8 for out_scale, bias, residual and the dropped lo * lo term (<= u S by
    construction of the planes: |lo| <= 2^-11 |hi|).  Count = 2 * terms * K / 32 + 8.
  fp32 (gemm_f32.hip): v_mfma_f32_32x32x2_f32 adds two products to its accumulator (charged one rounding each, the "fmaf chain" of the
    kernel's header).  The running sum is folded into a total every four k-tiles, so a chain holds at most 4 * 32 = 128 products and
    its roundings are bounded by u times the partial sums of ITS block; summed over the blocks that is min(K, 128) u S.  The folds add
    ceil(K / 128) roundings of at most u S, the last add, bias and residual three more.  Count = min(K, 128) + ceil(K / 128) + 3.
  GELU epilogues: the pre-activation bar times max |gelu'| <= 1.13, plus the activation's own error: 4 u |ref| for the erf form
    (loco_kernels.h: 2.2e-7 = 3.7 u relative); the tanh form (epilogue 5, x / (1 + 2^y)) adds 2 u |x|: y carries ~5 u relative
    error, which 2^y turns into 3.5 |y| u relative, and |x| e^-t * 5 t u <= 5 u |x| / e over t = y ln 2 > 0.
  Plane outputs: hi + lo is compared, and hi + lo keeps 22 bits: + 2^-21 |ref|.

Encoder attention (attention_f32.hip, attention_f16x3.hip), attention_bar() below.  out[i,d] = sum_j w_ij v_jd, w = softmax_j(s_ij + bias_ij)
over the valid keys; S[i,d] = sum_j w_ij |v_jd| with the fp64 softmax w.  Everything that perturbs a probability is first expressed as an
absolute error delta_ij of its score (a relative error of p_ij IS an absolute error of its exponent), then propagated:
  1. Score.  64-deep dot products: f16x3_count(64) = 20 roundings of at most u A_ij, A_ij = sum_c |q_c| |k_c| (the dropped lo * lo term is
     among the 8 of that count); the fp32 kernel f32_count(64) = 68, plus 2 for q * log2e (one rounding per element of q and the
     constant's own half ulp).  A table entry the kernel forms itself (the pe forms) carries f16x3_count(64) + 1 roundings (the + 1:
     * pe_scale is exact, the entry is then rounded once more when it is added) of u sum_c |q_c| |pe_c|; a table that is an INPUT is an
     operand and carries none.  Adding the bias to the score: one rounding, u (|s_ij| + |bias_ij|).
  2. Exponent argument.  f16x3: fma(s, log2e, (cb - m) log2e) -- cb - m rounded once, times log2e once, log2e itself half an ulp, the
     fma once: at most 4 u (|s_ij| + |m_i - cb|) in nats; the fp32 kernel (scores already in the log2 domain, mx + cb, cb - m, s + dsh)
     the same count.  m is a running maximum and cb one of the row's own biases, so |s_ij| + |m_i - cb| <= 2 (max_j |s_ij| + max_j |bias_ij|).
     v_exp_f32: one ulp = 2 u relative.
  3. Propagation.  With p_ij (1 + delta_ij) in numerator and denominator the output moves by sum_j w_ij delta_ij (v_jd - out_id), at most
     sum_j w_ij delta_ij (|v_jd| + |out_id|) <= 2 max_j delta_ij * S[i,d]   (|out| <= S).
  4. P V accumulation.  f16x3: 2 * terms * 4 = 24 roundings per 64-key tile (four 16-key steps of three MFMAs, two roundings each, as in
     the GEMM count) plus one for the rescale by alpha: 25 * ntiles, each at most u S (partial sums of |p v| / l never exceed S).  fp32:
     32 MFMAs of two products per tile and accumulator, one rounding per product, plus the rescale: 65 * ntiles.
  5. Dropped terms (f16x3 only).  P_lo V_lo is never formed and P = hi + lo keeps 22 bits: 2^-21 S each.
  6. Normalisation.  l = sum_j p_ij is a sum of positive terms, so its error is relative: at most 32 additions and one rescale per tile
     and lane half, one addition across the halves, 1 / l and the final product: (33 * ntiles + 4) u |ref|.
  7. Plane outputs: + 2^-21 |ref|, as above.
Charged nothing: alpha and the running maximum.  p, l and O all carry the factor exp(-m) for whatever m the kernel holds; an error in
m or in alpha = exp(m_old - m_new) scales numerator and l_run by the SAME rounded number (both are multiplied by the one alpha register),
and the quotient does not see it.  What an inexact m does cost is the |m_i - cb| of part 2, which is charged there.
ntiles = ceil(frames[b] / 64) of the clip.  Bar = [2 max_j delta_ij + (pv * ntiles + dropped) u] S + parts 6 and 7.

Attention probabilities (attention_probs.hip), probs_bar() below.  P_ij = exp(S_ij - m_i) / l_i over the valid keys j < n, S = s + bias in
nats.  As above, every error of an exponent's argument is an absolute error delta_ij of the score in nats and a relative error of p_ij;
first order in u throughout.  Each count is read off the kernel's instruction sequence (the `scores` lambda, pass 1, the reduction, pass 2):
  1. delta_ij, the `scores` lambda and the exponential of pass 2:
     a. the product s_ij: u A_ij, A_ij = sum_c |q_c| |k_c|, times the count of the form.  f32: 32 v_mfma_f32_32x32x2_f32 in ONE chain (no
        fold), each adding two products, one rounding per product: 64.  x3: four 16-deep k-steps of three v_mfma_f32_32x32x16_f16, two
        roundings each as in the GEMM count: 24; the dropped Q_lo K_lo is at most 2^-22 (1 + 2^-10) A (|lo| <= 2^-11 |hi|): 5 more, 29.
        x2: four k-steps of two MFMAs, 16; its reference (Q_hi + Q_lo) K_hi drops exactly the terms the kernel drops, so nothing more.
        The fp16 products themselves are exact in fp32.
     b. a table entry the f16x3 attention launch formed (the chained form): (f16x3_count(64) + 1) u sum_c |q_c| |pe_c|, part 1 of the
        attention bar.  A table that is an input is an operand: nothing.  A row that reads no entry (i >= n + 158) has bias 0 exactly.
     c. `acc + bias`: one rounding, u (|s_ij| + |bias_ij|).
     d. `* kLog2e`: the constant's own rounding and the product's, 2 u |S_ij| (a relative error of the log2 score is the same relative
        error of the score in nats).
     e. `acc - m` in pass 2: one rounding of the difference, u |S_ij - m_i|.  m_i itself is one of the rounded scores, bit for bit the
        same number in pass 1 and pass 2 (the rounding barrier at the end of `scores`); as in the attention bar it is charged nothing.
     f. v_exp_f32: one ulp, 2 u.
  2. Pass 1 sees the SAME rounded scores, so parts a-d perturb numerator and l_i alike and l_i's share is their p-weighted mean: at most
     max_j delta_ij.  Part e has a counterpart: key j enters l through exp2(s - mn) and is then rescaled by exp2(m_old - m_new) once per
     later tile and by exp2(m_lane - m_row) in the reduction; the running maximum only rises, so the rounded differences along that
     chain telescope to at most u (m_i - S_ij), the same bound.  Hence |dP_ij| <= P_ij (2 max_j delta_ij + c_norm u) + FLT_MIN, the
     FLT_MIN for a result v_exp_f32 or the final product may flush.
  3. c_norm, what is left of l_i's roundings and the final product: per 32-key tile of pass 1, `l * exp2(m - mn) + exp2(s - mn)`: the
     rescale's v_exp_f32 (2 u), its product and the addition: 4 per tile, ceil(n / 32) tiles; the reduction's `l * exp2(m - mr)` (v_exp_f32
     and product: 3) and the 5 additions of the butterfly (d = 16 ... 1); `1.0f / lr` (one ulp at worst: 2); `exp2(.) * l` in pass 2 (1).
     c_norm = 4 ceil(n / 32) + 11.  (The first key's exponential in l is part 1 f's counterpart; it is counted in row sums below.)
  4. Row sums.  sum_j P_ij = (sum_j p2_ij) / l_i with p2 the exponentials of pass 2 and l_i the sum pass 1 formed of ITS exponentials
     of the same scores: the score errors a-d cancel exactly, what remains is part e on both sides, the two v_exp_f32 (2 u each), c_norm
     and one FLT_MIN per key: |sum_j P_ij - 1| <= (2 max_j |S_ij - m_i| + 4 + c_norm) u + n FLT_MIN.
  5. The context made of these probabilities, sum_j P_ij v_jd in fp64: within sum_j bar_ij |v_jd| of the fp64 context, which is at most
     (2 max_j delta_ij + c_norm u) S[i,d] + n FLT_MIN max |v|, so within that plus the attention bar of what the attention kernel returns.
Scores of +-inf or NaN are outside the contract (include/loco_asr.h): exp2(inf - inf) is NaN.

Skinny GEMM (decoder.hip: skinny_gemm_kernel), skinny_count() below; S as for the GEMMs above.  ks = skinny_slices(N, K), which restates
the launcher's skinny_gemm_slices in Python (a test that disagrees with the launcher about ks only moves the bar by a few counts; the values
are checked either way).  A lane's partial sum is one chain of 4 FMAs per 256-element chunk over the chunks of its slice, ceil(K / 256 / ks)
of them in slice 0, which holds the most; wave_sum adds 6 roundings (the butterfly, d = 32 ... 1), the merge of the slices in LDS ks - 1,
the bias one and the residual one.  Every partial sum is a sum of a subset of the products, so each rounding is at most u S.
Count = 4 ceil(K / 256 / ks) + 6 + (ks - 1) + 2.  The GELU epilogue is the erf form of the GEMMs above (the same gelu_erf): element_bar().

Decoder attention (decoder.hip: dec_attention_kernel, dec_attention_combine; decoder_common.h: LOCO_DEC_LOAD_Q, LOCO_DEC_QK,
LOCO_DEC_SOFTMAX_TILE), dec_attention_bar() below.  out[i,d] = sum_j w_ij v_jd, w = softmax_j(s_ij) over the keys visible to query i,
s_ij = sum_c (scale q_c) k_c; S[i,d] = sum_j w_ij |v_jd| with the fp64 softmax w.  As for the encoder's attention, every error of an
exponent's argument is an absolute error delta_ij of the score and a relative error of p_ij:
  1. Score.  `q * scale`: one rounding per element of q, u A_ij in the sum, A_ij = sum_c |scale q_c| |k_c|.  LOCO_DEC_QK: four partial sums of
     16 FMAs each, combined as (a0 + a1) + (a2 + a3): an element's product passes 16 + 2 roundings of at most u A_ij.  19 u A_ij.
  2. `sc - m_new`: one rounding of the difference, u |s_ij - m| with m the running maximum of the tile, s_ij <= m <= m_i: at most
     u (m_i - s_ij), m_i the row's maximum.
  3. expf is OCML's, not v_exp_f32.  No HIP math document with ULP figures ships with this ROCm installation, so it is charged 2 ulp =
     4 u relative.  (A cap, not a measurement: what this bar exists for -- a dropped or extra key, a wrong row, a lost chunk -- moves an
     element by orders of magnitude more.)
  4. Splits (nsplit > 1), dec_attention_combine: a split's sum and O are both multiplied by w = expf(ms - m).  It is the same register in
     numerator and denominator, like corr below; it is charged all the same, as an error of the scores of the split's keys: the
     difference's rounding, u |ms - m| <= u max_j (m_i - s_ij), and expf's 4 u.
  5. Propagation, as in part 3 of the encoder's bar: 2 max_j delta_ij * S[i,d].
  6. P V.  Per tile of 64 keys `o *= corr` and up to 64 FMAs: 65 roundings, each at most u S once divided by l (partial sums of |p v| / l never
     exceed S); per split one FMA in the combine.  (65 ntiles + nsplit) u S, ntiles = ceil(n_i / 64) with n_i the visible keys of the
     query: splits begin at multiples of 64, so the tiles of all splits together are the tiles of the row.
  7. Normalisation.  l is a sum of positive terms, its error relative: per tile `s_run * corr` (1), the 6 additions of wave_sum(p) and the
     sum (1); per split one FMA; the final division: (8 ntiles + nsplit + 1) u |ref|.
Charged nothing: the running maximum and corr = expf(m_run - m_new).  o and s_run are multiplied by the ONE corr register, so whatever
it holds scales numerator and denominator alike, and p, s_run and o all carry the factor exp(-m) for whatever m the wave holds.  What an
inexact m costs is part 2.  A query without a visible key is outside the bar: its output is exactly 0.0 and is asserted as such.
Bar = [2 max_j delta_ij + (65 ntiles + nsplit) u] S + (8 ntiles + nsplit + 1) u |ref|, nsplit = 0 in both brackets without splits.

The waveform front end (tests/frontend_cases.py, tests/test_gpu_frontend_contract.py); e = 2^-53.
Normaliser (norm_misc.hip: wav_moments_kernel, wav_norm_coeffs_kernel, wav_norm_apply_kernel), normalize_bar() below.
out = (x - mean) * rstd for i < n, the padding value's bits for i >= n.
  1. `(float) mean`: one rounding, u |mean|; `xb[i] - mean`: one, u |x - mean|; both are then multiplied by rstd.
  2. `(float)(1.0 / sqrt(var + 1e-7))` and the product: one rounding each, 2 u |ref|.
  3. rstd's own error, relative, from var = q / n - mean^2 in fp64.  A sample's square or the sample passes `depth` roundings on its way
     into q or s: the product v * v (1), a thread's chain of ceil(chunk / 256) additions (chunk = ceil(n / 128) rounded up to 4), the 8
     levels of the shared-memory tree and the 128 parts in sequence.  q is a sum of positive terms: relative error depth e, one more
     for / n.  s: depth e sum |x|, one more for / n, and |mean| and mean |x| are both at most sqrt(q / n), so mean^2 moves by at most
     (2 (depth + 1) + 1) e q / n; the subtraction adds one.  |d var| <= (3 depth + 5) e q / n.  rstd = (var + 1e-7)^-1/2 halves the
     relative error; sqrt and the division add one rounding each: c = (3 depth + 5) / 2 + 2, charged as c e (q / n) / (var + 1e-7) |ref|.
     The clamp var > 0 only moves var towards its true value.
conv0 + GroupNorm + GELU (conv0_gn_gelu.hip), conv0_bar() below.  h = fma(y - mu, sc, be), y the chain of 10 fmaf, Y = sum_k |w_k| |x_k|.
  1. y: 10 roundings of at most u Y; `(float) mean`: u |mu|; `y - mu`: u |y - mu|; all times |sc|.
  2. `(float)(gn_w / sqrt(var + eps))`: u |sc| |y - mu|; the fma: u |h|.
  3. sc's error from var = E[y^2] - mean^2 in fp64.  The kernel never sums y^2: it forms w^T M w from 55 second moments of the strided
     waveform, whose terms have both signs, so the scale of its roundings is not E[y^2] but sum_kk' |w_k| |w_k'| |M_kk'| <= E[Y^2].
     A moment passes depth = 1 (the product) + ceil(per / 256) (a thread's chain, per = ceil(T0 / 64)) + 6 (butterfly) + 2 (the four
     waves) + 64 (the parts in sequence) + 1 (/ T0) roundings; the quadratic form adds 2 for the products w_k w_k' M and 55 for its
     chain: (depth + 57) e E[Y^2].  mean: (depth + 11) e E[Y], |mean| <= E[Y] <= sqrt(E[Y^2]), so mean^2 moves by (2 (depth + 11) + 1) e
     E[Y^2]; the subtraction one more.  |d var| <= (3 depth + 81) e E[Y^2]; halved by the root, plus sqrt and the division:
     c = (3 depth + 81) / 2 + 2, charged as c e E[Y^2] / (var + eps) |sc| |y - mu|.  (The issue's sketch charged E[y^2]; E[Y^2] is
     what the instruction sequence supports.)
  4. erf GELU as in element_bar: 1.13 * bar + 4 u |ref|.  The u |h| of part 2 matters here: for x < 0 gelu_erf's own error is up to
     1.0 u |x| absolute (value_domain_cases.RESTATED_NEG_ABS_PER_X), more than 4 u |ref| in the tail, but |gelu'| <= 0.13 there, so
     0.13 bar + u |h| <= 1.13 bar.  Planes: + max(2^-21 |ref|, 2^-25), planes_bar(): lo is an fp16 number, subnormal below 2^-14
     with spacing 2^-24, so hi + lo misses a small value by up to 2^-25 absolute.  (The planes themselves are held to the bits of the
     fp32 form's split; this bar only says what hi + lo is worth.)
  The statistics run over the launch's whole T0 (zero tail included), or over t0_clip[b] frames; frames at and beyond t0_clip[b] are +0.0.
Positional conv, fp32 (pos_conv.hip), pos_conv_count below.  ONE accumulator per element takes all K = 128 x 48 = 6144 products, four per
v_mfma_f32_16x16x4_f32 (one per lane quarter), never folded: one rounding per product as in the fp32 GEMM's count, K of them, each at
most u S, S = sum |h| |w| + |bias|; `acc + bv` one more, and two spare for the order inside an MFMA: K + 3.  Then the erf GELU rule
and the two additions `hv + gelu + table`: 2 u (|h| + |gelu| + |table|).  Per product the bar is loose (S / 6144 at K + 3 roundings of
u S), per tap it is not (S / 128): frontend_cases' one-hot weights make the conv a single exact product, and the bar a few u.
"""
import math

import numpy as np
import torch

from conftest import record_figure
from gpu_util import check, lib, ptr, stream

U = 2.0 ** -24
SENTINEL = {torch.float32: 0x7FC0BEEF, torch.float16: 0x7E5A}  # quiet NaNs with a payload
_INT = {torch.float32: torch.int32, torch.float16: torch.int16}
TILE_SLACK = 256  # rows (and elements) of sentinel behind every output: one full 256 x 256 tile


class Layout:
    """nb1 x nb2 matrices of rows x cols inside one flat allocation: element (z1, z2, r, c) at head + z1 s1 + z2 s2 + r ld + c,
    `head` elements of guard before and `tail` after (default: 256 rows and 256 elements)."""

    def __init__(self, rows, cols, ld=None, nb1=1, nb2=1, s1=0, s2=0, head=64, tail=None):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.nb1, self.nb2, self.s1, self.s2, self.head = nb1, nb2, s1, s2, head
        self.tail = TILE_SLACK * self.ld + TILE_SLACK if tail is None else tail
        self.span = (nb1 - 1) * s1 + (nb2 - 1) * s2 + (rows - 1) * self.ld + cols
        self.total = self.head + self.span + self.tail
        self._index = None

    def index(self):
        """flat positions of the owned elements, int64 [nb1, nb2, rows, cols] on the device"""
        if self._index is None:
            ar = lambda n: torch.arange(n, device="cuda", dtype=torch.int64)
            self._index = (self.head + ar(self.nb1)[:, None, None, None] * self.s1 + ar(self.nb2)[None, :, None, None] * self.s2 +
                           ar(self.rows)[None, None, :, None] * self.ld + ar(self.cols)[None, None, None, :])
            assert self._index.unique().numel() == self._index.numel(), "layout overlaps itself"
        return self._index


class Subset:
    """An owned set that is no matrix: `positions` (int64, flat, relative to element 0 of the region, all below `span`) inside an
    allocation of head + span + tail elements.  Usable wherever a Layout is, as one row of len(positions) columns."""

    def __init__(self, positions, span, head=64, tail=TILE_SLACK * 320 + TILE_SLACK):
        self.nb1 = self.nb2 = self.rows = 1
        self.cols = int(positions.numel())
        self.head, self.span, self.tail = head, span, tail
        self.total = head + span + tail
        self._index = (positions.to(device="cuda", dtype=torch.int64) + head).view(1, 1, 1, -1)

    def index(self):
        return self._index


def sentinel_buffer(layout, dtype):
    return torch.full((layout.total,), SENTINEL[dtype], dtype=_INT[dtype], device="cuda").view(dtype)


def base(buf, layout):
    """pointer to element (0, 0, 0, 0)"""
    import ctypes
    return ctypes.c_void_p(buf.data_ptr() + layout.head * buf.element_size())


def poisoned(values, layout):
    """values [nb1, nb2, rows, cols] (device) placed in a NaN-filled allocation of the layout"""
    buf = torch.full((layout.total,), float("nan"), dtype=values.dtype, device="cuda")
    buf[layout.index().reshape(-1)] = values.reshape(-1)
    return buf


def owned(buf, layout):
    return buf[layout.index().reshape(-1)].view(layout.nb1, layout.nb2, layout.rows, layout.cols)


def assert_guards(buf, layout, what=""):
    """every element outside the layout still holds the sentinel, every element inside was written"""
    bits = buf.view(_INT[buf.dtype])
    sent = SENTINEL[buf.dtype]
    mask = torch.ones(layout.total, dtype=torch.bool, device="cuda")
    mask[layout.index().reshape(-1)] = False
    touched = torch.nonzero(mask & (bits != sent)).reshape(-1)
    assert touched.numel() == 0, f"{what}: {touched.numel()} guard elements overwritten, first at flat offset {int(touched[0]) - layout.head}"
    unwritten = int((owned(bits, layout) == sent).sum())
    assert unwritten == 0, f"{what}: {unwritten} owned elements never written"


def split_planes(x):
    """fp32 device tensor -> (hi, lo) fp16 planes by the library's own split kernel"""
    x = x.contiguous()
    hi = torch.empty(x.shape, dtype=torch.float16, device="cuda")
    lo = torch.empty_like(hi)
    check(lib().loco_op_split_f16(ptr(x), ptr(hi), ptr(lo), x.numel(), stream()))
    return hi, lo


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu_new64(x):
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def f16x3_count(K, terms=3):
    return 2 * terms * K / 32 + 8


def f32_count(K):
    return min(K, 128) + math.ceil(K / 128) + 3


def products(a, w, out_scale=1.0):
    """a [..., M, K], w [N, K] or [..., N, K], fp64 on the CPU: (a w^T, |a| |w|^T) times out_scale -- computed once per operand pair and
    shared by every epilogue's reference, never modified"""
    wt = w.transpose(-1, -2)
    return out_scale * (a @ wt), out_scale * (a.abs() @ wt.abs())


def reference(a, w, bias=None, R=None, epilogue=0, out_scale=1.0, prod=None):
    """The operands the kernel really multiplies (a, w as in products, or prod = products(a, w, out_scale)), bias [N] / R [..., M, N] or
    None, all fp64 on the CPU.  Returns (ref, pre, S): the epilogue's result, its pre-activation argument and the forward-error scale."""
    pre, S = prod if prod is not None else products(a, w, out_scale)
    if bias is not None:
        pre = pre + bias
        S = S + bias.abs()
    if epilogue == 2:
        pre = pre + R
        S = S + R.abs()
    ref = gelu64(pre) if epilogue == 1 else gelu_new64(pre) if epilogue == 5 else pre
    return ref, pre, S


def element_bar(ref, pre, S, count, epilogue=0, planes=False):
    bar = count * U * S
    if epilogue in (1, 5):
        bar = 1.13 * bar + 4 * U * ref.abs()
    if epilogue == 5:
        bar = bar + 2 * U * pre.abs()
    if planes:
        bar = bar + 2.0 ** -21 * ref.abs()
    return bar


EPS64 = 2.0 ** -53


def normalize_cancel_count(n):
    """c of the normaliser's part 3 for a row of n samples"""
    chunk = (math.ceil(n / 128) + 3) // 4 * 4
    depth = 1 + math.ceil(chunk / 256) + 8 + 128
    return (3 * depth + 5) / 2 + 2


def normalize_bar(x, ref, mean, var, q_over_n, rstd, n):
    """The normaliser's bar of the docstring for one row's samples x (fp64), ref = (x - mean) rstd; mean, var, q_over_n, rstd fp64 scalars"""
    bar = rstd * U * (abs(mean) + (x - mean).abs()) + 2 * U * ref.abs()
    return bar + normalize_cancel_count(n) * EPS64 * q_over_n / (var + 1e-7) * ref.abs()


def conv0_cancel_count(T0):
    """c of conv0's part 3 for statistics over T0 frames"""
    depth = 1 + math.ceil(math.ceil(T0 / 64) / 256) + 6 + 2 + 64 + 1
    return (3 * depth + 81) / 2 + 2


def planes_bar(bar, ref):
    """a bar for hi + lo of a value written as fp16 planes: the + 2^-21 |ref| of the docstring, levelling off at 2^-25 where lo is a
    subnormal fp16 number (spacing 2^-24 whatever |ref| is: value_domain_cases.split_bound) -- conv0's GELU output has such elements"""
    return bar + (2.0 ** -21 * ref.abs()).clamp_min(2.0 ** -25)


def conv0_bar(ref, h, y, Y, mu, sc, var, EY2, T0, eps=1e-5):
    """conv0's bar of the docstring.  ref, h, y, Y [..., T, 512]; mu, sc, var, EY2 = E[Y^2] broadcastable per (clip, channel); T0 the
    frames the statistics ran over (a number or a tensor broadcastable like mu).  Planes: planes_bar() of this."""
    d = (y - mu).abs()
    c = conv0_cancel_count(T0) if not torch.is_tensor(T0) else torch.as_tensor(
        [conv0_cancel_count(int(t)) for t in T0.reshape(-1)], dtype=torch.float64).reshape(T0.shape)
    rel_sc = U + c * EPS64 * EY2 / (var + eps)
    pre = sc.abs() * U * (10 * Y + mu.abs() + d) + rel_sc * sc.abs() * d + U * h.abs()
    return 1.13 * pre + 4 * U * ref.abs()


POS_CONV_K = 128 * 48
pos_conv_count = POS_CONV_K + 3


def pos_conv_bar(g, pre, S, h, tab, count=pos_conv_count):
    """The fp32 positional conv's bar: g = gelu(pre), S the conv's scale, h and tab the two addends, all fp64 of one shape"""
    return element_bar(g, pre, S, count, 1) + 2 * U * (h.abs() + g.abs() + tab.abs())


def attention_bar(kernel, ref, S, A_max, P_max, s_max, b_max, ntiles, table_formed, planes=False):
    """The attention bar of the docstring.  kernel "f32" or "f16x3"; ref, S [B, 12, T, 64]; per query row [B, 12, T, 1]: A_max = max_j sum_c
    |q_c| |k_c|, P_max = max_j sum_c |q_c| |pe_c| of the table entries its valid keys read, s_max = max_j |s_ij|, b_max = max_j |bias_ij|;
    ntiles [B, 1, 1, 1]; table_formed: the kernel computes the table itself (pe planes given)."""
    x3 = kernel == "f16x3"
    delta = (f16x3_count(64) if x3 else f32_count(64) + 2) * U * A_max
    if table_formed:
        delta = delta + (f16x3_count(64) + 1) * U * P_max
    delta = delta + U * (s_max + b_max)               # score + bias
    delta = delta + 4 * U * 2 * (s_max + b_max) + 2 * U  # exponent argument, v_exp_f32
    bar = 2 * delta * S + (25 if x3 else 65) * ntiles * U * S
    if x3:
        bar = bar + 2 * 2.0 ** -21 * S
    bar = bar + (33 * ntiles + 4) * U * ref.abs()
    if planes:
        bar = bar + 2.0 ** -21 * ref.abs()
    return bar


def skinny_slices(N, K):
    """skinny_gemm_slices of decoder.hip, restated: the k-slices a (N, K) product is launched with"""
    chunks = K // 256
    if chunks >= 8 or (N <= 128 and chunks >= 4):
        return 4
    return 2 if chunks >= 2 else 1


def skinny_count(N, K, bias=True, residual=False):
    ks = skinny_slices(N, K)
    return 4 * math.ceil(K / 256 / ks) + 6 + (ks - 1) + int(bias) + int(residual)


def dec_attention_splits(B, Sq, Tk):
    """dec_attention_splits of decoder.hip, restated: (splits, keys per split) of a launch_dec_attention"""
    rows = B * 12 * Sq
    ns = max(1, min((4096 + rows - 1) // rows, (Tk + 255) // 256, 64))
    return ns, ((Tk + ns - 1) // ns + 63) // 64 * 64


def dec_pool_attention_splits(Tk_bound):
    """dec_pool_attention_splits of decoder.hip, restated: splits of 256 keys"""
    return 1 if Tk_bound <= 256 else (Tk_bound + 255) // 256


def dec_attention_bar(ref, S, A_max, spread_max, nvis, nsplit):
    """The decoder attention bar of the docstring.  ref, S [..., 64]; per query row [..., 1]: A_max = max_j sum_c |scale q_c| |k_c| and
    spread_max = max_j (m_i - s_ij) over the visible keys, nvis their number; nsplit the launch's key splits (1: no combine)."""
    ntiles = torch.ceil(nvis / 64)
    split = nsplit if nsplit > 1 else 0
    delta = (19 * A_max + spread_max + 4) * U
    if split:
        delta = delta + (spread_max + 4) * U
    return (2 * delta + (65 * ntiles + split) * U) * S + (8 * ntiles + split + 1) * U * ref.abs()


FLT_MIN = 2.0 ** -126
PROBS_PRODUCT_COUNT = {"f32": 64, "x3": 29, "x2": 16}


def probs_bar(form, P, s, bias, A, valid, n, table_abs=None):
    """The probabilities bar of the docstring.  form "f32", "x3" or "x2"; P the fp64 softmax, s, bias, A = sum_c |q_c| |k_c| [B, 12, T, T];
    valid bool [B, 1, 1, T]; n [B, 1, 1, 1] valid keys per clip; table_abs: sum_c |q_c| |pe_c| of each key's entry where the attention
    launch formed the table, else None.  -> (bar [B, 12, T, T], rel [B, 12, T, 1] = 2 max_j delta_ij + c_norm u, the row sums' bar
    [B, 12, T, 1])."""
    S = s + bias
    m = S.masked_fill(~valid, float("-inf")).amax(-1, keepdim=True)
    delta = PROBS_PRODUCT_COUNT[form] * U * A                       # a
    if table_abs is not None:
        delta = delta + (f16x3_count(64) + 1) * U * table_abs       # b
    delta = delta + U * (s.abs() + bias.abs())                      # c
    delta = delta + 2 * U * S.abs()                                 # d
    spread = (S - m).abs().masked_fill(~valid, 0.0)
    delta = delta + U * spread + 2 * U                              # e, f
    c_norm = 4 * torch.ceil(n / 32) + 11
    rel = 2 * delta.masked_fill(~valid, 0.0).amax(-1, keepdim=True) + c_norm * U
    row_sum_bar = (2 * spread.amax(-1, keepdim=True) + 4 + c_norm) * U + n * FLT_MIN
    return P * rel + FLT_MIN, rel, row_sum_bar


def assert_elements(name, out, ref, S, bar, rel_l2_bar=None, **tags):
    """out within bar of ref element by element (and rel_l2 below rel_l2_bar); the measured maximum of err / (u S) is recorded"""
    out = out.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(out).all()), f"{name} {tags}: {int((~torch.isfinite(out)).sum())} non-finite outputs"
    err = (out - ref).abs()
    ratio = float((err / (U * S)).max())
    worst = float((err / bar).max())
    rl2 = float((out - ref).norm() / ref.norm())
    record_figure(name, max_err_over_uS=round(ratio, 3), max_err_over_bar=round(worst, 4), rel_l2=float(f"{rl2:.3e}"), **tags)
    print(f"{name} {tags}: max err / (u S) = {ratio:.3f}, max err / bar = {worst:.4f}, rel_l2 = {rl2:.3e}")
    if worst > 1.0:
        at = np.unravel_index(int(torch.argmax(err / bar)), tuple(ref.shape))
        raise AssertionError(f"{name} {tags}: element {at} is {worst:.3g} x its bar (err {float(err[at]):.3e}, u S {U * float(S[at]):.3e}); "
                             f"{int((err > bar).sum())} elements over")
    if rel_l2_bar is not None:
        assert rl2 < rel_l2_bar, f"{name} {tags}: rel_l2 {rl2:.3e} >= {rel_l2_bar}"
    return ratio


def assert_dec_attention(name, out, r, nsplit, **tags):
    """out [B, 12, Sq, 64] against r, the dict of decoder_contract_cases.attn_reference: a query without a visible key holds exactly 0.0,
    every other element is within dec_attention_bar of the fp64 reference"""
    out = out.detach().cpu().reshape(r["ref"].shape)
    has = r["has_keys"].expand_as(r["ref"])
    empty = out[~has]
    assert bool((empty == 0).all()), f"{name} {tags}: {int((empty != 0).sum())} elements of queries without a key are not 0.0 (NaN: {int(empty.isnan().sum())})"
    if not bool(has.any()):
        return 0.0
    bar = dec_attention_bar(r["ref"], r["S"], r["A_max"], r["spread_max"], r["nvis"], nsplit)
    return assert_elements(name, out[has], r["ref"][has], r["S"][has], bar[has], **tags)


def same_bits(a, b):
    return int((a.view(_INT[a.dtype]) != b.view(_INT[b.dtype])).sum()) == 0


class knobs:
    """with knobs(LOCO_GEMM_TILE="3"): ...  -- sets the A/B knobs of gemm_f16x3.hip (or LOCO_ATTN_LONG), reloads them, and restores the environment and
    reloads again on the way out, also after a failure."""

    def __init__(self, **env):
        self.env = {k: v for k, v in env.items() if v is not None}

    def __enter__(self):
        import os
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update({k: str(v) for k, v in self.env.items()})
        lib().loco_debug_reload_gemm_knobs()
        return self

    def __exit__(self, *exc):
        import os
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib().loco_debug_reload_gemm_knobs()
        return False
