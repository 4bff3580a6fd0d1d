// Internal launcher declarations shared by the kernel translation units and the C-ABI (loco_api.hip).
// gfx950 only: 64-lane wavefronts, fp32-input MFMA (v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace loco {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kHidden = 768;
constexpr int kHeads = 12;
constexpr int kHeadDim = 64;
constexpr int kFfn = 3072;
constexpr int kConvDim = 512;
constexpr int kPosK = 128;
constexpr int kPosGroups = 16;
constexpr int kPosCg = 48;  // channels per group
constexpr int kRelMax = 160;
constexpr int kRelN = 320;
constexpr int kQkv = 3 * kHidden;

// Workspace of the split-K path: ks * tiles_m * tiles_n <= 256 tiles of at most 256 x 128 partial sums.
constexpr size_t kSplitKBytes = (size_t)256 * 256 * 128 * sizeof(float);
constexpr int kSplitKMaxM = 8192;

enum Epilogue { kEpiNone = 0, kEpiGelu = 1, kEpiResidual = 2, kEpiQkvScatter = 3, kEpiPosConv = 4, kEpiGeluNew = 5 };

struct GemmArgs {
    const float* A;
    const float* W;
    const float* bias;  // may be null
    const float* R;     // residual (kEpiResidual), same batch strides as C
    float* C;
    int M, N, K;
    long lda, ldw, ldc, ldr;
    int nb1, nb2;
    long sA1, sA2, sC1, sC2;
    int epilogue;
};

// split-precision GEMM operands: fp16 hi/lo planes with the strides of the fp32 tensor they stand for
struct GemmSplitArgs {
    const _Float16* Ahi;
    const _Float16* Alo;
    const _Float16* Whi;
    const _Float16* Wlo;
    const float* bias;  // may be null
    const float* R;     // fp32 residual (kEpiResidual)
    float* C;           // fp32 output, or null when Chi/Clo are given
    _Float16* Chi;      // split output (the next GEMM's A operand), or null
    _Float16* Clo;
    int M, N, K;
    long lda, ldw, ldc, ldr;
    int nb1, nb2;
    long sA1, sA2, sC1, sC2;
    int epilogue;
    // kEpiQkvScatter (fused q|k|v projection feeding the split-precision attention): columns [0,768) -> Chi/Clo planes
    // [M,768] (q), [768,1536) -> the k planes, [1536,2304) -> the v planes, each pair qkv_stride halves behind the previous one (attention
    // transposes V with its LDS read)
    // kEpiResidual: the residual may also be given as fp16 hi/lo planes (same element offsets and ldr as R); it is then hi + lo,
    // exact in fp32.  The encoder's residual stream lives only in that form between layers (LayerNorm writes no fp32 copy); the
    // encoder itself hands these planes to the LayerNorm behind the GEMM (launch_layernorm's rhi / rlo) and launches kEpiNone.
    const _Float16* Rhi = nullptr;
    const _Float16* Rlo = nullptr;
    // split-K for small problems (launch_gemm_split decides): fp32 partial sums [ks][M][N], >= kSplitKBytes when set
    float* splitk_ws = nullptr;
    long qkv_stride = 0;  // kEpiQkvScatter: k planes at Chi / Clo + qkv_stride, v planes at + 2 qkv_stride (halves)
    int T = 0;
    // kEpiPosConv (grouped positional conv as a GEMM over the group-major halo layout, see launch_group_major_split):
    // z1 = clip, z2 = group; C = R + GELU(acc + bias) + sin_table[pos(t)], pos = t+2 for t < frames[z1] else 1
    // The weight planes hold W * 2^k (k chosen per tensor at load time so that max|W| lands in [2^13, 2^14): fp16's 5-bit
    // exponent then serves the weights' own spread instead of their absolute level); the accumulator is multiplied by
    // out_scale = 2^-k before bias / activation -- exact, a power of two.
    float out_scale = 1.0f;
    int terms = 3;  // 3: A_hi W_hi + A_lo W_hi + A_hi W_lo;  2: the W_lo term dropped (precision mode "f16x2")
    // true while another stream of the same forward is launching kernels of its own (the two half-batch schedule): a partly filled
    // last round is then filled by that stream's workgroups, and the tile choice stops paying for whole rounds
    bool co_scheduled = false;
    // Convolution as a GEMM over overlapping rows (A row t = input rows stride*t .. stride*t + ktaps - 1, K = ktaps * C): with
    // ktaps > 1 the k axis is walked (64-channel block, tap slot, 32-channel half), tap slots in the order 0, 2, 1, and the weight
    // planes are stored in that order (launch_permute_conv_k).  An input row that is tap 2 of output t is tap 0 of output t+1
    // (stride 2): in a tap-major walk its two uses are 32 k-tiles apart, by when 1.5 MB per CU have gone through the XCD's
    // 4 MiB L2 and the row is fetched again (conv1: 1.5 x its 6.3 GB operand).  Here they are two k-tiles apart, and the two
    // 64-byte halves of every 128-byte line are consecutive k-tiles.
    int ktaps = 1;
    int kchan = 0;       // channels per tap (0: K / ktaps); set by the split-K path, whose slices see only part of K
    int kt_per_z2 = 0;   // split-K with ktaps > 1: slice z2 starts at k-tile z2 * kt_per_z2 of that walk (its A offset is not linear)
    // Range tracking: where the output is written as fp16 hi/lo planes, max|x| of what was written is folded into
    // range_slot[0..7] (see range_commit); null = not tracked.
    float* range_slot = nullptr;
    long sW2 = 0;                   // weight stride per z2 (0 = shared weights)
    // z1 may itself be a pair (outer, inner), z1 = outer * z1_inner + inner: sA1 then strides the outer part, sA1i / sW1i the inner
    // one (C still strides the combined z1).  Used by the split-K path of the grouped positional conv, whose batch dimensions
    // (clip, group) are both taken: inner = K slice.
    int z1_inner = 1;
    long sA1i = 0, sW1i = 0;
    long sBias2 = 0;                // bias stride per z2
    const float* sin_table = nullptr;
    const int32_t* frames = nullptr;
};
// x [B,T,768] fp32 -> fp16 hi/lo planes in group-major layout [B][16][T+128][48] with 64 zero frames before and after:
// output frame t of group g then reads the CONTIGUOUS run rows t .. t+127 (128 taps x 48 channels = K 6144, lda = 48)
// rows_clip (device, [B], may be null): packed forward -- rows t >= rows_clip[b] of clip b read as zeros (the conv's zero padding
// starts where the clip's own reference batch ends)
hipError_t launch_group_major_split(const float* x, void* hi, void* lo, int B, int T, hipStream_t s, float* range_slot = nullptr,
                                    const int32_t* rows_clip = nullptr);
// folded positional-conv weight [g][tap][o][i] -> [g][o][tap*48 + i] (the GEMM's W, ldw = 6144)
hipError_t launch_pos_w_for_gemm(const float* wf, float* out, hipStream_t s);
hipError_t launch_attention_f16x3(const _Float16* qhi, const _Float16* qlo, const _Float16* khi, const _Float16* klo,
                                  const _Float16* vhi, const _Float16* vlo, const float* qp, const int32_t* frames,
                                  _Float16* ctx_hi, _Float16* ctx_lo, float* ctx, int B, int T, hipStream_t s,
                                  const _Float16* pe_hi = nullptr, const _Float16* pe_lo = nullptr, float pe_scale = 1.0f);
// pe_hi / pe_lo != nullptr: the relative-position table is COMPUTED by the kernel (Qp = q . pe_k^T * pe_scale, pe planes [320][64])
// into `qp`, which is then scratch of the launch ([B,12,T,320] fp32) instead of an input.
hipError_t launch_gemm_split(const GemmSplitArgs& a, hipStream_t s);
void reload_gemm_knobs();  // re-read the LOCO_GEMM_* A/B knobs from the environment (gemm_f16x3.hip)
void reload_attention_knobs();  // ... and LOCO_ATTN_LONG (attention_f16x3.hip)
// hi/lo planes of x * scale (scale a power of two)
hipError_t launch_split_f16(const float* x, void* hi, void* lo, long n, hipStream_t s, float scale = 1.0f);
// max |x| over n elements -> *out (one float, device); out must be zeroed by the caller
hipError_t launch_absmax(const float* x, long n, float* out, hipStream_t s);

// diagnostics: count the non-finite elements of a buffer (out[0] += count, out[1] = min(first index)); LOCO_DEBUG_NONFINITE=1
hipError_t launch_count_nonfinite(const void* x, long n, bool half, unsigned long long* out, hipStream_t s);

// ---- range tracking of tensors stored as fp16 hi/lo planes (precision mode f16x3) ------------------------------------------
// hi = fp16(x) is inf from |x| >= 65520 on, and the pair (hi, lo) keeps 22 significant bits only while lo = fp16(x - hi) is a
// normal fp16 number, i.e. for |x| >~ 2^-3; below that the ABSOLUTE error levels off at 2^-25.  A tensor is therefore
// represented to fp32 class relative to its own scale as long as its largest element sits well inside (2^-6, 65504) -- the
// range include/loco_asr.h guarantees.
//   * Tensors whose range follows from the weights alone are checked on the host, at no run-time cost: LayerNorm outputs
//     (|y| <= sqrt(D) max|gamma| + max|beta|), the attention context (a convex combination of V rows) -- loco_api.hip,
//     static_range_check.
//   * The unbounded ones -- conv0's GroupNorm + GELU output (its bound grows with sqrt(frames per clip): useless for 10-minute
//     clips), GELU outputs of conv layers 1-5 and of the feed-forward intermediate, q|k|v, the feature projection -- are tracked
//     where they are produced: the GEMM epilogue (and group_major_split) folds max|x| of what it
//     writes, taken on the fp32 value before conversion, into its stage's status word.  8 shards per stage (workgroup id mod
//     8) so that no single address takes every workgroup's atomic; the word is read EARLY (range_peek, before the epilogue's
//     arithmetic, so the load's latency is hidden) and a wave whose maximum is already covered skips the atomic -- the word
//     only grows, so a stale read costs at most a redundant atomic.  The wave maximum is taken with four DPP steps inside
//     the rows of 16 lanes and four v_readlane across them: no LDS traffic, no waits.
// The host reads the words after the forward (loco_forward_status) and decides (include/loco_asr.h).
constexpr int kRangeShards = 8;
constexpr int kRangeMaxStages = 96;
constexpr int kFiniteStage = kRangeMaxStages - 1;  // reserved: set to +inf by the forward's last LayerNorm when a row is not finite
__device__ __forceinline__ unsigned range_peek(const float* slot) {
    if (!slot) return 0xffffffffu;
    return __hip_atomic_load(reinterpret_cast<const unsigned*>(slot) + (blockIdx.x & (kRangeShards - 1)), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
}
// max over the wave's 64 lanes of a NON-NEGATIVE value (lanes without a partner read 0); every lane must be active
__device__ __forceinline__ float wave_max_nonneg(float v) {
#define LOCO_DPP_MAX(ctrl) \
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true)))
    LOCO_DPP_MAX(0xB1);   // quad_perm [1,0,3,2]: lane ^ 1
    LOCO_DPP_MAX(0x4E);   // quad_perm [2,3,0,1]: lane ^ 2
    LOCO_DPP_MAX(0x141);  // row_half_mirror: the other quad of each 8
    LOCO_DPP_MAX(0x140);  // row_mirror: the other half of each row of 16
#undef LOCO_DPP_MAX
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
// Sum / maximum over the wave's 64 lanes (all active, all left with the result): the xor butterfly with steps 32, 16, ..., 1, whose
// order is part of the result -- many tests compare bits -- and is written down here only.  T: float, double or int.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ void range_commit(float* slot, float amax, unsigned seen) {
    if (!slot) return;
    const unsigned bits = __float_as_uint(wave_max_nonneg(amax));  // non-negative floats order like their bit patterns; NaN never enters (fmaxf)
    if ((threadIdx.x & 63) == 0 && bits > seen)
        atomicMax(reinterpret_cast<unsigned*>(slot) + (blockIdx.x & (kRangeShards - 1)), bits);
}

// The same for kernels of MANY small workgroups (the split-K reductions: thousands of 256-thread blocks that all start at once
// and all peek a zero word): one atomic per workgroup instead of one per wave -- the wave maxima meet in LDS first.  Every thread
// of the block must call it.  (With one atomic per wave the reduction behind FFN1's split-K GEMM took 72 us at 498 rows, 50 of
// them in ~6 000 atomics on eight addresses: a quarter of a whole forward of the reference's 2 x 5 s batch.)
__device__ __forceinline__ void range_commit_block(float* slot, float amax, unsigned seen) {
    if (!slot) return;
    __shared__ float wmax[16];
    const float w = wave_max_nonneg(amax);
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = wmax[0];
        for (unsigned i = 1; i < (blockDim.x + 63) / 64; ++i) m = fmaxf(m, wmax[i]);
        const unsigned bits = __float_as_uint(m);
        if (bits > seen) atomicMax(reinterpret_cast<unsigned*>(slot) + (blockIdx.x & (kRangeShards - 1)), bits);
    }
}

// exact GELU 0.5*x*(1+erf(x/sqrt2))

// Exact (erf) GELU, HF transformers/activations.py:83-89, without erff's two divergent branches.
//   erfc(t) = exp(-t q(t)) for t >= 0 with q(t) = -ln(erfc(t)) / t smooth and slowly varying (q(0) = 2/sqrt(pi)); with
//   s = |x|, t = s/sqrt(2) and the 1/sqrt(2) and log2(e) factors folded into the coefficients:  e = 2^(-s Q(s)) = erfc(s/sqrt 2),
//   GELU(x) = x (1 - e/2) for x >= 0,   x e/2 for x < 0        -- no cancellation in either branch.
// Q: degree-9 fit of q on t in [0, 4.1] (erfc(4.1) = 6.7e-9; |x| is clamped there, GELU is x resp. 0 to 2e-8 beyond).
// Against an fp64 GELU on [-9, 9]: relative error <= 2.2e-7 for x > 0 (torch's fp32 GELU: 3.7e-7), absolute error <= the
// rounding of x itself; relative L2 on N(0, 1.5) inputs 2.9e-8.  10 FMAs + one v_exp_f32 instead of ~45 instructions.
__device__ __forceinline__ float gelu_erf(float x) {
    constexpr float kSMax = 5.79827547f;  // 4.1 * sqrt(2)
    const float s = fminf(fabsf(x), kSMax);
    float q = 2.171883651e-08f;
    q = fmaf(q, s, -6.759613029e-07f);
    q = fmaf(q, s, 9.013814633e-06f);
    q = fmaf(q, s, -6.522983313e-05f);
    q = fmaf(q, s, 2.421164681e-04f);
    q = fmaf(q, s, 7.379760791e-05f);
    q = fmaf(q, s, -7.028903347e-03f);
    q = fmaf(q, s, 5.248807371e-02f);
    q = fmaf(q, s, 4.592096508e-01f);
    q = fmaf(q, s, 1.151104808e+00f);
    const float h = 0.5f * __builtin_amdgcn_exp2f(-(q * s));  // erfc(|x| / sqrt 2) / 2
    // the clamp of the negative branch is a compare + select, not fmaxf: fmaxf(NaN, c) = c would launder a NaN input into a finite
    // number (HF's GELU propagates it, and the forward's finite check must see it)
    return x >= 0.f ? x * (1.0f - h) : (x < -kSMax ? -kSMax : x) * h;
}

// GPT-2's tanh GELU ("gelu_new", HF transformers/activations.py NewGELUActivation): 0.5 x (1 + tanh(u)), u = sqrt(2/pi) (x + 0.044715 x^3).
// tanh goes through exp2: tanh(u) = 1 - 2 / (1 + e^(2u)), so 0.5 (1 + tanh(u)) = 1 / (1 + e^(-2u)) and the result is x / (1 + 2^(-2 log2(e) u)).
// The exponential saturates to 0 or +inf, never inf / inf: tanh is exactly +-1 from |u| ~ 44 on, large positive x returns x, large negative
// finite x returns -0, and there is no 1 - tanh cancellation in the negative tail.  No fmaxf / fminf anywhere (see gelu_erf): NaN comes out
// as NaN, and so does -inf (HF's own -inf * 0), +inf as +inf.
__device__ __forceinline__ float gelu_new(float x) {
    const float u = 0.7978845608028654f * fmaf(0.044715f * x, x * x, x);
    return x / (1.0f + __builtin_amdgcn_exp2f(-2.885390081777927f * u));
}

// fp16 hi/lo split of two value pairs (a0,a1) and (b0,b1): hi = fp16(x) (hipcc emits one v_cvt_pk_f16_f32 per pair),
// lo = fp16(x - hi) by one mixed-precision FMA per value (fp32 x, fp16 hi: the difference is exact in fp32, so lo is
// rounded once -- bit for bit what `lo = (_Float16)(x - (float)hi)` gives, at 6 instructions for 4 values instead of 16).
//  * the inputs are pinned first: left to itself hipcc folds the producing multiply into v_fma_mix*_f16 for lo but converts
//    hi from the fp32-rounded product (one fp16 ulp of hi on ties);
//  * hi stays compiler-visible code, so the first instruction that reads a value coming from an MFMA or from the
//    transcendental unit is one hipcc pads itself -- it does not look inside inline asm;
//  * inside the asm the two pairs are interleaved: each v_fma_mixhi (which merges into the register its v_fma_mixlo wrote
//    16 bits of) has an independent instruction in front of it.
__device__ __forceinline__ void split_f16_2pairs(float a0, float a1, float b0, float b1, unsigned& hia, unsigned& loa, unsigned& hib,
                                                 unsigned& lob) {
    typedef _Float16 h2_ __attribute__((ext_vector_type(2)));
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1));
    const h2_ ha = {(_Float16)a0, (_Float16)a1}, hb = {(_Float16)b0, (_Float16)b1};
    hia = __builtin_bit_cast(unsigned, ha);
    hib = __builtin_bit_cast(unsigned, hb);
    asm("v_fma_mixlo_f16 %0, %2, 1.0, -%6 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %1, %4, 1.0, -%7 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %3, 1.0, -%6 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %5, 1.0, -%7 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(loa), "=&v"(lob)
        : "v"(a0), "v"(a1), "v"(b0), "v"(b1), "v"(hia), "v"(hib));
}

// The same on two values at once: the polynomial runs on v_pk_fma_f32 (two fp32 FMAs per instruction).
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_t gelu_erf2(f32x2_t x) {
    constexpr float kSMax = 5.79827547f;
    const f32x2_t s = {fminf(fabsf(x.x), kSMax), fminf(fabsf(x.y), kSMax)};
#define LOCO_Q2(c) (f32x2_t){(c), (c)}
    f32x2_t q = LOCO_Q2(2.171883651e-08f);
    q = __builtin_elementwise_fma(q, s, LOCO_Q2(-6.759613029e-07f));
    q = __builtin_elementwise_fma(q, s, LOCO_Q2(9.013814633e-06f));
    q = __builtin_elementwise_fma(q, s, LOCO_Q2(-6.522983313e-05f));
    q = __builtin_elementwise_fma(q, s, LOCO_Q2(2.421164681e-04f));
    q = __builtin_elementwise_fma(q, s, LOCO_Q2(7.379760791e-05f));
    q = __builtin_elementwise_fma(q, s, LOCO_Q2(-7.028903347e-03f));
    q = __builtin_elementwise_fma(q, s, LOCO_Q2(5.248807371e-02f));
    q = __builtin_elementwise_fma(q, s, LOCO_Q2(4.592096508e-01f));
    q = __builtin_elementwise_fma(q, s, LOCO_Q2(1.151104808e+00f));
#undef LOCO_Q2
    const f32x2_t u = q * s;
    const f32x2_t h = {0.5f * __builtin_amdgcn_exp2f(-u.x), 0.5f * __builtin_amdgcn_exp2f(-u.y)};
    f32x2_t r;
    r.x = x.x >= 0.f ? x.x * (1.0f - h.x) : (x.x < -kSMax ? -kSMax : x.x) * h.x;  // NaN-propagating clamp, see gelu_erf
    r.y = x.y >= 0.f ? x.y * (1.0f - h.y) : (x.y < -kSMax ? -kSMax : x.y) * h.y;
    return r;
}

hipError_t launch_gemm(const GemmArgs& a, hipStream_t s);
hipError_t launch_layernorm(const float* x, const float* g, const float* b, float* y, long rows, int dim, float eps,
                            hipStream_t s, void* yhi = nullptr, void* ylo = nullptr, float* nonfinite_slot = nullptr,
                            const void* rhi = nullptr, const void* rlo = nullptr);  // rhi / rlo: normalise x + (rhi + rlo), fp16 planes [rows, dim]

constexpr int kConv0Parts = 64;    // partial-moment blocks per clip
constexpr int kConv0Moments = 65;  // 10 first + 55 second moments
size_t conv0_scratch_bytes(int B);
hipError_t launch_conv0_gn_gelu(const float* wav, int B, long L, const float* w, const float* gn_w, const float* gn_b,
                                float* out, void* scratch, float eps, hipStream_t s, void* out_hi = nullptr,
                                void* out_lo = nullptr, float* range_slot = nullptr, const int32_t* t0_clip = nullptr);
// t0_clip (device, [B], may be null): packed forward -- GroupNorm statistics of clip b over its first t0_clip[b] conv frames only,
// frames beyond written as zeros
hipError_t launch_frame_counts(const int32_t* mask, int B, long L, int32_t* frames, hipStream_t s);
size_t normalize_scratch_bytes(int B);
hipError_t launch_normalize_waveform(const float* wav, const int32_t* mask, int B, long L, float pad, float* out, void* scratch,
                                     hipStream_t s);
hipError_t launch_token_counts(const int32_t* mask, int B, int T, int32_t* frames, hipStream_t s);
hipError_t launch_text_prenet(const int32_t* ids, const float* embed, int vocab, const float* alpha, const float* pe, int B, int T,
                              float* out, hipStream_t s);
hipError_t launch_text_pe_table(float* pe, int rows, hipStream_t s);
hipError_t launch_pos_conv(const float* h, const float* wf, const float* bias, const float* sin_table,
                           const int32_t* frames, float* out, int B, int T, hipStream_t s, const int32_t* rows_clip = nullptr);
hipError_t launch_attention(const float* qkv, const float* qp, const int32_t* frames, float* ctx, int B, int T,
                            hipStream_t s, void* ctx_hi = nullptr, void* ctx_lo = nullptr);
// attention_probs.hip: P[b,h,i,j] = softmax over the valid keys of q.k + qp (output_attentions), fp32 [B,12,T,T].  Exact-fp32 operands
// (qkv [B,T,2304], qhi == nullptr) or fp16 hi/lo planes of q and k ([B*T,768], `terms` 3 or 2 MFMA terms); qp as the layer's attention
// launch left it (include/loco_asr.h, loco_op_attention_probs*).
hipError_t launch_attention_probs(const float* qkv, const _Float16* qhi, const _Float16* qlo, const _Float16* khi, const _Float16* klo,
                                  const float* qp, const int32_t* frames, float* probs, int B, int T, int terms, hipStream_t s);

// weight preparation (run once in loco_finalize_weights)
hipError_t launch_relayout_conv_weight(const float* w, float* out, int N, int C, int k, hipStream_t s);  // [N,C,k]->[N,k*C]
hipError_t launch_fold_pos_conv(const float* g, const float* v, float* out, hipStream_t s);  // -> [16][128][48][48]
hipError_t launch_scale_copy(const float* src, float* dst, long n, float scale, hipStream_t s);
// conv weight [N][taps][C] (tap-major K) -> [N][C/64][tap slot][2][32] (the k order of GemmSplitArgs::ktaps; slots = taps 0, 2, 1)
hipError_t launch_permute_conv_k(const float* src, float* dst, int N, int taps, int C, hipStream_t s);
hipError_t launch_sinusoid_table(float* tab, int rows, hipStream_t s);

// sample-rate conversion (resample.hip)
int resample_design(int sr_in, int sr_out, int* L_out, int* M_out, int* K_out, float* taps);
hipError_t launch_resample(const float* x, int B, long n_in, long x_stride, const float* taps, int L, int M, int K, float* y, long n_out,
                           long y_stride, hipStream_t s);

// text decoder (decoder.hip)
constexpr int kDecStartToken = 2, kDecEosToken = 2, kDecPadToken = 1;  // SpeechT5Config: decoder_start_token_id, eos_token_id, pad_token_id
constexpr int kSkinnyMaxM = 64;        // rows of the weight-streaming GEMM (and clips of one decode step)
constexpr int kDecAttnMaxSplit = 64;   // key splits of one decoder attention launch
// C[m,n] = epi(sum_k A[m,k] W[n,k] + bias[n]) (+ R[m,n]); K % 256 == 0, lda / ldw % 4 == 0; columns n >= nsplit go to
// C2[m, n - nsplit] when C2 is given (the step's q | k|v product: q to a row buffer, k|v into the cache)
hipError_t launch_skinny_gemm(const float* A, long lda, const float* W, long ldw, const float* bias, const float* R, long ldr, float* C,
                              long ldc, float* C2, long ldc2, int nsplit, int M, int N, int K, int epilogue, hipStream_t s);
int skinny_gemm_slices(int N, int K);
int dec_attention_splits(int B, int Sq, int Tk);
size_t dec_attention_scratch_bytes(int B, int Sq, int Tk);
// out[b,i,h,:] = softmax_j(scale q[b,i,h,:] . k[b,j,h,:]) v[b,j,h,:] over keys j < kcount[b] (null: Tk) and, when causal,
// j <= i + causal_offset; ld* = row strides, s* = clip strides in floats; scratch >= dec_attention_scratch_bytes
hipError_t launch_dec_attention(const float* q, long ldq, long sq, const float* k, long ldk, long sk, const float* v, long ldv, long sv,
                                const int32_t* kcount, float* out, long ldo, long so, int B, int Sq, int Tk, int causal, int causal_offset,
                                float scale, float* scratch, hipStream_t s);
hipError_t launch_dec_embed(const int32_t* ids, long ld_ids, const float* embed, int vocab, const float* table, int table_rows, float* x,
                            int B, int S, int32_t* positions, hipStream_t s);
hipError_t launch_dec_embed_step(const int32_t* tokens, int S_max, int t, const float* embed, int vocab, const float* table, int table_rows,
                                 int32_t* nonpad, float* x, int B, hipStream_t s);
hipError_t launch_dec_select(const float* logits, int vocab, int B, int32_t* tokens, int S_max, int t, int32_t* finished, int32_t* lengths,
                             int32_t* state, int eos, int pad, hipStream_t s);
hipError_t launch_dec_begin(int32_t* tokens, int B, int S_max, int start, int pad, int32_t* lengths, int32_t* state, hipStream_t s);

// ---- decoder slot pool (decoder.hip: the row-scatter GEMM and the fixed-boundary attention; decoder_pool.hip: the slot state) ----
constexpr int kDecPoolSplitKeys = 256;  // split s of a pool attention covers keys [256 s, 256 s + 256)
constexpr int kPoolFree = 0, kPoolOpen = 1, kPoolFinished = 2;
// launch_skinny_gemm's kEpiNone form for M <= 64 rows whose C2 part of row m goes to C2[m ldc2 + c2_rows[m] c2_row_stride + ...]
// (c2_rows on the device; a negative entry drops the row's C2 part)
hipError_t launch_skinny_gemm_rows(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, float* C2,
                                   long ldc2, const int32_t* c2_rows, long c2_row_stride, int nsplit, int M, int N, int K, hipStream_t s);
int dec_pool_attention_splits(int Tk_bound);
size_t dec_pool_attention_scratch_bytes(int slots, int Tk_bound);
hipError_t launch_dec_pool_attention(const float* q, const float* k, long ldk, long sk, const float* v, const int32_t* kcount, float* out,
                                     int slots, int Tk_bound, float* scratch, hipStream_t s);
// Per-slot state, all i32 [slots] on the device: status (kPool*), pos (token the slot consumes next), cap, frames, lengths; poll[0] =
// slots open.  tokens is [slots, S_max].
struct PoolState {
    int32_t *poll, *status, *pos, *cap, *frames, *lengths, *tokens;
    int32_t *cur, *cnt;  // the token a slot consumes next and the non-pad tokens of its utterance up to and including it
    int32_t *self_count, *cross_count, *kv_row;  // what a step's embed kernel derives for the step's GEMM and attention launches
    int slots, S_max, T_cap;
};
struct PoolAdmit {  // by value: at most 64 clips
    int n;
    int32_t slot[kSkinnyMaxM], cap[kSkinnyMaxM], rows[kSkinnyMaxM];
};
hipError_t launch_pool_init(const PoolState& p, hipStream_t s);
hipError_t launch_pool_admit(const PoolState& p, const PoolAdmit& a, const int32_t* frames, int start, hipStream_t s);
hipError_t launch_pool_embed(const PoolState& p, const float* embed, int vocab, const float* table, int table_rows, float* x, int max_pos,
                             int max_frames, hipStream_t s);
hipError_t launch_pool_select(const PoolState& p, const float* logits, int vocab, int eos, hipStream_t s);

// ---- decoder sampling (decoder_sample.hip) ----
// temperature > 0, top_k >= 0 (0 = off), top_p in (0, 1] (1 = off), the Philox key = the seed's low and high word
struct SampleRule {
    float temperature;
    int top_k;
    float top_p;
    uint32_t key0, key1;
};
// tokens[m] = the rule's token for row m of logits (ld >= V; columns >= V are never read) with the Philox counter counters[m] =
// (utterance, hypothesis, t); greedy (optional) [M]: nonzero = the row's argmax.  keep (optional) i32 [M, V], uniform (optional) f32 [M].
hipError_t launch_sample_tokens(const float* logits, long ld, int M, int V, const SampleRule& rule, const uint32_t* counters, const int32_t* greedy,
                                int32_t* tokens, int32_t* keep, float* uniform, hipStream_t s);
struct PoolAdmitSamples {  // by value: at most 64 slots; slot i holds a hypothesis of clip i / copies
    int n, copies;
    int32_t slot[kSkinnyMaxM], cap[kSkinnyMaxM], rows[kSkinnyMaxM];
    uint32_t utterance[kSkinnyMaxM], hypothesis[kSkinnyMaxM];
};
// ids u32 [slots, 2] on the device: (utterance, hypothesis) of every slot admitted this way
hipError_t launch_pool_admit_samples(const PoolState& p, const PoolAdmitSamples& a, const int32_t* frames, int start, uint32_t* ids, hipStream_t s);
// launch_pool_select for a pool whose slots r with bit r of `sampled` set draw by the rule; step_tokens (optional) i32 [slots]
hipError_t launch_pool_sample_select(const PoolState& p, const uint32_t* ids, unsigned long long sampled, const SampleRule& rule, const float* logits,
                                     int vocab, int eos, int32_t* step_tokens, int ignore_index, hipStream_t s);

// ---- decoder beam search (decoder_beam.hip) ----
constexpr int kBeamMax = 16;  // beams of one group
// K beams per group, early: 0 false, 1 true, 2 "never"; penalty_positive = (length_penalty > 0), all the device needs of it beside den
struct BeamRule {
    int K, early, penalty_positive;
};
// What a beam pool keeps beside PoolState; group g owns slots g K .. g K + K - 1.  Per slot: run f64 (accumulated score), alive i32,
// tlp f32 [slots, S_max] (entry t = log P of token t of the slot's row, entry 0 = 0), parent i32 (the slot whose rows 0 .. count - 1
// the slot takes over after the step) and count i32.  Per group: unsat i32, fin_n i32 and the finished list, best first, entry e of
// group g at index g K + e: fin_score f64, fin_sum f64, fin_len i32, fin_tok i32 [., S_max], fin_tlp f32 [., S_max].
// den f64 [den_n]: den[n] = n ** length_penalty, computed on the host.
struct BeamState {
    double *run, *fin_score, *fin_sum;
    const double* den;
    float *tlp, *fin_tlp;
    int32_t *alive, *parent, *count, *unsat, *fin_n, *fin_len, *fin_tok;
    int groups, den_n;
};
// groups of a.copies = K slots: PoolAdmitSamples' slot list (a.utterance, a.hypothesis unused), slot i the beam i % K of its group
hipError_t launch_pool_admit_beams(const PoolState& p, const BeamState& b, const PoolAdmitSamples& a, const int32_t* frames, int start, hipStream_t s);
// One step of the rule for every group whose first slot is open with kv_row >= 0 (the row the step wrote); logprobs f32 [slots, V] =
// the log-softmax rows the rule used.  Rows of logits at logits + r * ld.  Ends with poll[0] = slots open.
// bonus (optional) f64 [slots, V]: candidate (k, v) scores (run[k] + lp[k][v]) + bonus[k][v]; null is the rule without it, the same code
hipError_t launch_beam_select(const PoolState& p, const BeamState& b, const BeamRule& rule, const float* logits, long ld, int V, int eos,
                              float* logprobs, hipStream_t s, const double* bonus = nullptr);
// buf [layers][slots][S][W] of 4-byte words: rows 0 .. count[r] - 1 of slot r := those of slot parent[r] (clamped into r's group of K
// slots), through shadow (same shape), for every r whose parent differs and, with open (optional, [slots]), whose open[r] is
// kPoolOpen; max_count bounds the launches, not the copies
hipError_t launch_beam_reorder(void* buf, void* shadow, int layers, int slots, int S, long W, const int32_t* parent, const int32_t* count,
                               const int32_t* open, int K, int max_count, hipStream_t s);

// ---- n-gram language model over the decoder's ids (ngram.hip; the rule: include/loco_asr.h) ----
constexpr int kNgramMaxOrder = 8, kNgramMaxVocab = 127;
constexpr long kNgramMaxGrams = 1L << 26;
// A gram of `len` symbols (oldest first, the predicted one last; a symbol is 0 .. V, V = <s>) as one key: 7 bits per symbol from bit 0
// up, len in bits 56 .. 59.  Never 0, the mark of an empty slot.
__host__ __device__ inline uint64_t ngram_key(uint64_t symbols, int len) { return symbols | ((uint64_t)len << 56); }
// where a key's probe sequence starts (splitmix64's finaliser); host and device share it
__host__ __device__ inline uint64_t ngram_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
// The table on the device: open addressing with linear probing, mask + 1 slots (a power of two, at least twice the grams);
// vals[slot] = (logp, backoff).  No key's probe sequence is longer than max_probe slots, so a lookup ends whatever memory holds.
struct NgramTable {
    const uint64_t* keys;
    const double* vals;  // [mask + 1][2]
    uint32_t mask;
    int max_probe, V, order;
};
// out f64 [R, V]: row r = log P(v | the last min(order - 1, n) symbols of tokens[r * ld ..]), n = cur[r] + cur_offset the tokens the row
// holds (index 0 counts as <s>).  fuse: out = weight * log P + token_bonus (each rounded once) and a row whose n is outside 1 .. S is
// skipped; otherwise such a row, and a row with a context token outside 0 .. V - 1, is NaN.
hipError_t launch_ngram_logprobs(const NgramTable& t, const int32_t* tokens, long ld, int S, const int32_t* cur, int cur_offset, int R, bool fuse,
                                 double weight, double token_bonus, double* out, hipStream_t s);
// out f64 [total]: sequence b = tokens[starts[b] .. starts[b] + lens[b]); out[starts[b] + i] = log P(token i | tokens 0 .. i - 1), 0 at i = 0;
// a sequence that does not lie inside [0, total) is skipped
hipError_t launch_ngram_score(const NgramTable& t, const int32_t* tokens, const int64_t* starts, const int32_t* lens, int B, int64_t total,
                              double* out, hipStream_t s);

// ---- decoder scores (decoder_score.hip) ----
// logprob[m] = log_softmax(logits[m, :V])[target] with target = targets[m], or the row's argmax (decoder_common.h's rule) when targets is
// null; 0 where targets[m] == ignore_index, NaN for another target outside [0, V); chosen (optional) [M] = the target used
hipError_t launch_token_logprob(const float* logits, long ld, const int32_t* targets, long M, int V, int ignore_index, float* logprob,
                                int32_t* chosen, hipStream_t s);
// seq_logprob[b] / seq_count[b] (optional) = sum / number of the positions of sequence b whose target is not ignore_index (null targets:
// all); loss[0] (optional) = -(sum over b) / (count over b), accumulated in double in an order that depends on (B, S) only
hipError_t launch_score_reduce(const float* logprob, const int32_t* targets, int B, int S, int ignore_index, float* seq_logprob,
                               int32_t* seq_count, float* loss, hipStream_t s);

// ---- decoder attention probabilities and token alignment (decoder_probs.hip) ----
constexpr int kDecAlignMaxTokens = 450;  // token rows of one DTW workgroup (max_text_positions)
// P[b,h,i,j] f32 [B,12,Sq,Tk] = softmax_j(scale q[b,i,h,:] . k[b,j,h,:]) over keys j < kcount[b] (null: Tk) and, when causal, j <= i;
// every other entry exactly 0 and its key row never read; ld* = row strides, s* = clip strides in floats
hipError_t launch_dec_attention_probs(const float* q, long ldq, long sq, const float* k, long ldk, long sk, const int32_t* kcount, float* P,
                                      int B, int Sq, int Tk, int causal, float scale, hipStream_t s);
// A[b,s,t] = (first ? 0 : A[b,s,t]) + sum of P[b,h,s,t] over the heads h whose bit is set in `heads`, ascending; times inv_n when last
hipError_t launch_dec_attn_mean(const float* P, float* A, int B, int S, int T, unsigned heads, int first, int last, float inv_n, hipStream_t s);
// monotone DTW over -A[b, s < n[b], t < frames[b] (null: T)] in double (row stride ld floats): start / end i32 [B,S] = each token's
// first frame and last frame + 1 on the path, -1 for s >= n[b]; back >= B * S * T bytes of back-pointers; S <= kDecAlignMaxTokens
hipError_t launch_dtw_align(const float* A, long ld, const int32_t* n, const int32_t* frames, int B, int S, int T, int32_t* start, int32_t* end,
                            unsigned char* back, hipStream_t s);

// ---- long-form segmentation (segment.hip) ----
constexpr int kVadHop = 320, kVadWindow = 400;  // the encoder's frame t covers samples [320 t, 320 t + 400)
constexpr int kVadBins = 512;                   // 0.25 dB bins from -120 dB
constexpr long kVadMaxFrames = 1L << 24;        // frames of one recording (93 hours)
constexpr int kVadNormal = 0, kVadSilent = 1, kVadAllSpeech = 2;
struct VadArgs {  // by value; everything the host derives from LocoVadParams and F
    int F, max_frames, min_frames, min_silence, min_speech, pad, trim;
    int k_noise, k_peak;  // ceil(quantile * F), in 1 .. F
    float margin_db, abs_floor_db, min_dynamic_db;
    int max_segments;
};
constexpr int kVadMaxChannels = 8;
// wav [C, stride] -> db [C, F]: db[c][t] = 10 log10(mean of x^2 over frame t of row c + 1e-12) for t < F = (n - 80) / 320; n >= 400,
// stride >= n.  A mono recording is C = 1.
hipError_t launch_frame_energy_db(const float* wav, int C, long n, long stride, float* db, hipStream_t s);
// one workgroup per channel, with the cross-talk gate between channels (segment.hip): db [C, F] -> seg_start / seg_end / overlap (null:
// not computed, no second launch) i32 [C, max_segments], count i32 [C] (negative: -needed > max_segments), threshold_db f32 [C] (+inf:
// silent channel, -inf: no usable silence), all on the device; ws >= vad_channels_workspace_bytes(C, F).  A mono recording is C = 1 with
// crosstalk_db = +inf, and touches no more than vad_workspace_bytes(F) of ws.
size_t vad_workspace_bytes(long F);
size_t vad_channels_workspace_bytes(int C, long F);
hipError_t launch_vad_segments(const float* db, int C, const VadArgs& a, float crosstalk_db, int32_t* seg_start, int32_t* seg_end, int32_t* overlap,
                               int32_t* count, float* threshold_db, void* ws, hipStream_t s);

// ---- GPT-2 language-model scorer (lm.hip) ----
constexpr int kLmChunk = 1024;  // vocabulary columns of one lm_head_nll workgroup: fixed, part of the result's bits
int lm_head_chunks(int V);
size_t lm_head_scratch_bytes(long R, int V);
// nll[r] = logsumexp_{v < V}(h[r] . wte[v]) - h[r] . wte[targets[r]]; 0 where targets[r] == ignore_index, NaN for another target outside
// [0, V).  h [R, 768] (row stride ldh), wte [V, 768] (row stride ldw); scratch >= lm_head_scratch_bytes(R, V).  A row's result does not
// depend on R or on the row's index.
hipError_t launch_lm_head_nll(const float* h, long ldh, const float* wte, long ldw, const int32_t* targets, long R, int V, int ignore_index,
                              float* nll, void* scratch, hipStream_t s);
// x[b,s,:] = wte[tokens[start[b] + s]] + wpe[s] for s < len[b], zeros beyond; an id outside [0, V) embeds as zeros and lowers status[0]
// (optional; the caller sets it to INT_MAX) to its position in tokens
hipError_t launch_lm_embed(const int32_t* tokens, const int32_t* start, const int32_t* len, const float* wte, int V, const float* wpe, float* x,
                           int B, int S, int32_t* status, hipStream_t s);
// out[r,:] = x[rows[r],:] (rows = b S + s) and targets[r] = tokens[start[b] + s + 1], ignore_index where s + 1 >= len[b]
hipError_t launch_lm_gather(const float* x, const int32_t* rows, const int32_t* tokens, const int32_t* start, const int32_t* len, int B, int S,
                            int R, int ignore_index, float* out, int32_t* targets, hipStream_t s);
hipError_t launch_lm_transpose(const float* in, float* out, int rows, int cols, hipStream_t s);  // out[c][r] = in[r][c]
// mean[g] (double) = mean of nll[offsets[g] .. offsets[g + 1]) summed in double in an order that depends on the two offsets only; ppl = exp
hipError_t launch_lm_group_mean(const float* nll, const int32_t* offsets, int G, double* mean, double* ppl, hipStream_t s);

// ---- GPT-2 with a cached context (lm_attention.hip) ----
constexpr int kLmCtxMaxSeqs = 64;  // sequences of one call
constexpr int kLmCtxScore = 1, kLmCtxCommit = 2;
// By value.  Sequence n owns packed rows [row0[n], row0[n] + len[n]) of the call's buffers (sequence order, no gaps), its ids are
// tokens[tok0[n] ..], and it reads (and, with kLmCtxCommit, extends) cache slot slot[n], which holds P[n] tokens.
struct LmCtxSeqs {
    int n;
    int32_t row0[kLmCtxMaxSeqs], len[kLmCtxMaxSeqs], slot[kLmCtxMaxSeqs], P[kLmCtxMaxSeqs], tok0[kLmCtxMaxSeqs], flags[kLmCtxMaxSeqs];
};
// out[row0[n] + t, 64 h ..] = softmax_j(q . k_j / 8) v_j over the slot's cached keys j < P[n] and the sequence's own keys t' <= t.  qkv:
// packed rows of q | k | v (row stride 2304); kcache / vcache: [slot][position][768] with slot_stride floats between slots; out: row
// stride 768.  A sequence's output does not depend on n, on the other sequences or on the slot's index.
hipError_t launch_lm_ctx_attention(const float* qkv, const float* kcache, const float* vcache, long slot_stride, const LmCtxSeqs& seqs, float* out,
                                   hipStream_t s);
// x[row0[n] + t, :] = wte[tokens[tok0[n] + t]] + wpe[P[n] + t]; a bad id embeds as zeros and lowers status[0] to its index in tokens
hipError_t launch_lm_ctx_embed(const int32_t* tokens, const LmCtxSeqs& seqs, const float* wte, int V, const float* wpe, float* x, int32_t* status,
                               hipStream_t s);
// the k | v rows of the sequences with kLmCtxCommit -> cache positions P[n] + t of their slots
hipError_t launch_lm_ctx_append(const float* qkv, const LmCtxSeqs& seqs, float* kcache, float* vcache, long slot_stride, hipStream_t s);
// The R = sum of len over the sequences with kLmCtxScore scored rows, flat in sequence order: token t > 0 is predicted from x's row t - 1,
// token 0 from last[slot] (ignore_index and a zero row when the slot is empty)
hipError_t launch_lm_ctx_gather(const float* x, const int32_t* tokens, const LmCtxSeqs& seqs, const float* last, int R, int ignore_index, float* hsel,
                                int32_t* targets, hipStream_t s);
// last[slot[n], :] = x's last row of every sequence with kLmCtxCommit
hipError_t launch_lm_ctx_last(const float* x, const LmCtxSeqs& seqs, float* last, hipStream_t s);

// ---- edit distance and n-best risk (edit_distance.hip) ----
constexpr int kEditMaxLen = 16384;  // symbols per side: cost and S of a cell stay below 2^16, the row state below 64 KiB
// counts[p] = S, D, I, hits of the pair spans[p] = ref_start, ref_len, hyp_start, hyp_len into `symbols` (minimum cost, then most
// correct symbols); -1 x 4, nothing of the pair read, for a negative length, a length above kEditMaxLen, a span outside
// [0, n_symbols) or min(ref_len, hyp_len) > max_len.  max_len (0 .. kEditMaxLen) sizes the launch's LDS row state.  One wave per pair;
// a pair's numbers depend on its own two spans alone.
hipError_t launch_edit_distance(const int32_t* symbols, long n_symbols, const int32_t* spans, int P, int max_len, int32_t* counts, hipStream_t s);
// Group u holds hypotheses group_offsets[u] .. group_offsets[u + 1]; `counts` holds every group's N (N - 1) / 2 pairs (i < j) row-major,
// group after group.  risk[h] = sum over h' != h (ascending) of w[h'] cost(h, h') / sum over h' (ascending) of w[h'] in double, each
// product and sum rounded on its own; weights null = all 1; best[u] = the first index of least risk (-1 for an empty group).
hipError_t launch_nbest_risk(const int32_t* counts, const int32_t* group_offsets, const double* weights, int U, double* risk, int32_t* best,
                             hipStream_t s);

// ---- embedding neighbours (neighbors.hip) ----
constexpr int kTopkMaxK = 16;      // entries of a query's list: the lists of a 128-query workgroup take 16 KiB of LDS
constexpr int kTopkChunk = 1024;   // keys of one topk workgroup: fixed, part of the merge order
constexpr int kTopkDot = 0, kTopkCosine = 1, kTopkL2 = 2;
long topk_chunks(long N);
size_t topk_scratch_bytes(long M, long N, int k);  // 0 outside the limits
// n2[r] = the squared norm of x's row r (768 values, row stride ldx), summed in double in one order, rounded to fp32 once
hipError_t launch_row_norm2(const float* x, long ldx, long rows, float* n2, hipStream_t s);
// The k best keys of every query, best first, ties towards the lower key index: values f32 [M, k], indices i32 [M, k]; (-inf, -1) where
// fewer than k candidates exist.  dot: q.k; cosine: ((q.k) / max(|q|, 1e-12)) / max(|k|, 1e-12); l2: (2 q.k - |k|^2) - |q|^2.  qn2 / kn2
// (launch_row_norm2; unused for dot) are the squared norms; exclude (nullable) names one key per query that is no candidate (-1: none);
// a NaN score is no candidate.  scratch >= topk_scratch_bytes(M, N, k).  A query's result does not depend on M or on the query's row.
hipError_t launch_topk(const float* Q, long ldq, const float* K, long ldk, const float* qn2, const float* kn2, const int32_t* exclude, long M,
                       long N, int k, int metric, float* values, int32_t* indices, void* scratch, hipStream_t s);
// out[g, :] = the mean of rows[index[j], :] (index null: rows[j, :]) over j in [offsets[g], offsets[g + 1]), sums in double in an order
// that depends on the group's size alone, rounded to fp32 once; count[g] (nullable) = the group's size.  An empty group leaves out[g]
// as it is; a row index outside [0, n_rows) is not read and makes its group's mean NaN.
hipError_t launch_group_mean(const float* rows, long ld, long n_rows, const int32_t* index, const int64_t* offsets, long G, float* out, long ldo,
                             int32_t* count, hipStream_t s);

// the C ABI's error string (loco_last_error) for translation units other than loco_api.hip
int api_fail(int code, const char* fmt, ...);

inline long conv_out_len(long n, int k, int s) { return n < k ? 0 : (n - k) / s + 1; }

}  // namespace loco
