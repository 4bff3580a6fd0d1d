// C ABI (include/loco_asr.h), the encoder forward and its host-side orchestration: plans and workspace carve, the prenet and encoder
// schedules of both precision families, the enqueue around them (status block, two half-batches on two streams), every
// loco_forward* entry, the text front end and the workspace sizes.
//
// One forward = SpeechT5EncoderWithSpeechPrenet.forward in eval mode (HF modeling_speecht5.py:1339-1358):
//   prenet (HF :534-566): conv0+GroupNorm+GELU -> 6 x (conv as GEMM + GELU) -> LayerNorm(512) -> Linear(512,768)
//                         -> + GELU(pos-conv) + sinusoid
//   encoder (HF :1234-1322): LayerNorm(768) -> 12 x [ fused QKV GEMM, Qp GEMM, flash attention, out-proj GEMM(+x),
//                            LayerNorm, FFN1 GEMM(+GELU), FFN2 GEMM(+h), LayerNorm ]
// Everything is enqueued on the caller's stream from a caller-owned workspace; no allocation, host
// synchronisation or thread is used inside loco_forward (the one exception, growing the sinusoid table
// past its reserved rows, mirrors HF's own auto-grow at modeling:331-333 and is done before any launch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <mutex>
#include <utility>

#include "loco_host.h"

using namespace loco;
using namespace loco::host;

namespace {

// device side of the same: the first bytes of every workspace
constexpr size_t kStatusDevBytes = (sizeof(float) * kRangeMaxStages * kRangeShards + 255) & ~size_t(255);

// Per-call state of one loco_forward*: everything the enqueue mutates lives here, not in the handle, so that forwards of one
// handle may be enqueued from several host threads and be in flight together (different streams, workspaces and status blocks).
struct Call {
    int precision = 1;
    float* splitk = nullptr;     // split-K workspace of the (half-)batch being enqueued (null for large problems)
    bool dual = false;           // inside the two half-batch schedule (GemmSplitArgs::co_scheduled)
    float* range_dev = nullptr;  // [kRangeMaxStages][kRangeShards] in the workspace, zeroed at the start of the forward
    StatusBlock* st = nullptr;
    int nslot = 0;               // range slots taken by the (half-)batch being enqueued: each half starts again at 0
    // range tracking: one status word (x 8 shards) per tensor that is stored as fp16 planes and whose range does not follow from
    // the weights alone (loco_kernels.h), in launch order; the two halves of a dual-stream forward walk the same sequence and
    // share the words (a maximum does not care who contributes)
    float* slot(const char* name, int layer = -1) {
        if (!range_dev || !st || nslot >= kFiniteStage) return nullptr;
        st->names[nslot] = name;
        st->layer[nslot] = layer;
        return range_dev + (size_t)kRangeShards * nslot++;
    }
};

struct Plan {
    int B;
    long L;
    long Tc[7];  // conv output lengths
    long T, M;
    size_t off_frames, off_clip, off_c0scratch, off_a, off_b, off_x0, off_x1, off_tmp, off_ctx, off_qkv, off_qp, off_ffn, off_xs0, off_xs1,
        off_splitk, total;
    bool splitk;
};

void carve_plan(const loco_encoder* e, Plan& p);

bool make_plan(const loco_encoder* e, int B, long L, Plan& p) {
    p.B = B;
    p.L = L;
    long n = L;
    for (int i = 0; i < 7; ++i) {
        n = conv_out_len(n, kConvK[i], kConvS[i]);
        p.Tc[i] = n;
    }
    if (B <= 0 || n <= 0) return false;
    p.T = n;
    p.M = (long)B * n;
    carve_plan(e, p);
    return true;
}

// the text front end enters the encoder with T tokens per sequence: no waveform, no conv buffers
bool make_plan_tokens(const loco_encoder* e, int B, long T, Plan& p) {
    p.B = B;
    p.L = 0;
    for (int i = 0; i < 7; ++i) p.Tc[i] = 0;
    if (B <= 0 || T <= 0) return false;
    p.T = T;
    p.M = (long)B * T;
    carve_plan(e, p);
    return true;
}

void carve_plan(const loco_encoder* e, Plan& p) {
    const int B = p.B;
    const size_t f = sizeof(float);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o += align_up(bytes);
        return at;
    };
    p.off_frames = take((size_t)B * sizeof(int32_t));
    p.off_clip = take((size_t)3 * B * sizeof(int32_t));  // packed forward: per-clip conv0 / encoder frame counts (StatusBlock::clip_tab)
    p.off_c0scratch = take(conv0_scratch_bytes(B));
    p.off_a = take((size_t)B * p.Tc[0] * kConvDim * f);
    p.off_b = take((size_t)B * p.Tc[1] * kConvDim * f);
    p.off_x0 = take((size_t)p.M * kHidden * f);
    p.off_x1 = take((size_t)p.M * kHidden * f);
    p.off_tmp = take((size_t)p.M * kHidden * f);
    p.off_ctx = take((size_t)p.M * kHidden * f);
    // fp32 [M,2304], or (precision f16x3) q, k and v as fp16 hi|lo planes [M,768] each: the same bytes
    p.off_qkv = take((size_t)3 * p.M * kHidden * f);
    p.off_qp = take((size_t)p.M * kHeads * kRelN * f);
    // FFN intermediate [M,3072]; doubles as scratch for the group-major positional-conv operand [B,16,T+128,48] x 2 planes
    const size_t ffn_elems = (size_t)p.M * e->cfg.ffn, posg_elems = (size_t)B * (p.T + kPosK) * kHidden;
    p.off_ffn = take((ffn_elems > posg_elems ? ffn_elems : posg_elems) * f);
    p.off_xs0 = take((size_t)p.M * kHidden * f);  // fp16 hi|lo planes of x0 / x1 (precision f16x3)
    p.off_xs1 = take((size_t)p.M * kHidden * f);
    p.splitk = p.M <= kSplitKMaxM;  // small problems: fp32 partial sums of the split-K GEMM path (gemm_f16x3.hip)
    p.off_splitk = take(p.splitk ? kSplitKBytes : 0);
    p.total = o;
}

// Split-precision GEMM (A and W as fp16 hi/lo planes; output fp32 C or planes Chi/Clo) of one batch over dense rows (lda = ldw = K,
// ldc = N): callers set the operands by field name, and whatever strides or batches differently.
GemmSplitArgs split_args(int M, int N, int K, int epilogue) {
    GemmSplitArgs a{};
    a.M = M; a.N = N; a.K = K;
    a.lda = a.ldw = K;
    a.ldc = N;
    a.epilogue = epilogue;
    a.nb1 = a.nb2 = 1;
    return a;
}

// The one launch path of a split GEMM of the forward: the weight planes and every field that follows from the call are set here.
int run_gemm_split(loco_encoder* e, const Call& c, hipStream_t s, GemmSplitArgs a, const SplitW& w, int kid, double flops, double bytes) {
    a.Whi = w.hi;
    a.Wlo = w.lo;
    a.out_scale = w.inv_scale;
    a.terms = c.precision == 2 ? 2 : 3;
    a.co_scheduled = c.dual && a.epilogue != kEpiPosConv;  // never set for the positional conv, whose launch takes no tile choice from it
    a.splitk_ws = c.splitk;
    Bracket br(e, s, kid, flops, bytes);
    HIP_TRY(launch_gemm_split(a, s));
    return LOCO_OK;
}
int run_gemm_split(loco_encoder* e, const Call& c, hipStream_t s, const GemmSplitArgs& a, const SplitW& w) {
    return run_gemm_split(e, c, s, a, w, K_GEMM_SPLIT, gemm_flops(a.M, a.N, a.K, a.nb1, a.nb2),
                          gemm_bytes(a.M, a.N, a.K, a.nb1, a.nb2, a.epilogue));
}

// Diagnostics, off unless the environment had LOCO_DEBUG_NONFINITE=1 when the handle was created: after each stage of the f16x3
// forward, count the non-finite elements of what it wrote (host synchronisation per stage!) and name the FIRST stage that produced
// any on stderr.  The range words cannot see NaNs (fmaxf drops them); this can.
int dbg_check(loco_encoder* e, hipStream_t s, const char* stage, int layer, const void* p, size_t n, bool half, long row_len) {
    if (!e->debug_nonfinite || !p) return LOCO_OK;
    unsigned long long h[2] = {0, ~0ull};
    HIP_TRY(hipMemcpyAsync(e->debug_counter, h, sizeof h, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_count_nonfinite(p, (long)n, half, e->debug_counter, s));
    HIP_TRY(hipMemcpyAsync(h, e->debug_counter, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h[0])
        fprintf(stderr, "[loco debug] non-finite values: %llu of %zu elements written by '%s' (layer %d); first at element %llu = row %llu, column %llu\n",
                h[0], n, stage, layer, h[1], row_len ? h[1] / row_len : 0ull, row_len ? h[1] % row_len : 0ull);
    return LOCO_OK;
}
// the hi, then the lo plane of one tensor of n elements; `stage` holds one %s for "hi" / "lo"
void dbg_planes(loco_encoder* e, hipStream_t s, const char* stage, int layer, const _Float16* hi, const _Float16* lo, size_t n,
                long row_len) {
    if (!e->debug_nonfinite) return;
    char name[96];
    snprintf(name, sizeof name, stage, "hi");
    dbg_check(e, s, name, layer, hi, n, true, row_len);
    snprintf(name, sizeof name, stage, "lo");
    dbg_check(e, s, name, layer, lo, n, true, row_len);
}

}  // namespace

namespace loco::host {

// On success *tab is a table of at least `rows` rows: the snapshot this forward uses from here on, whatever other threads publish later.
int ensure_sin_rows(loco_encoder* e, int rows, hipStream_t s, const float** tab) {
    if (e->sin_rows.load(std::memory_order_acquire) >= rows) {
        // the count is stored AFTER its table: a table loaded now is that one or a later, longer one
        *tab = e->sin_tab.load(std::memory_order_acquire);
        return LOCO_OK;
    }
    // grow (HF does the same on demand, modeling:331-333); happens once per new maximum length.  Safe with other forwards of the handle
    // in flight: the new table is complete before it is published (this is the one place a forward may block its host thread), and
    // the old one is RETIRED, not freed -- forwards already enqueued on other streams keep reading it -- until loco_destroy.
    std::lock_guard<std::mutex> lock(e->sin_mu);
    if (e->sin_rows.load(std::memory_order_relaxed) >= rows) {
        *tab = e->sin_tab.load(std::memory_order_relaxed);
        return LOCO_OK;
    }
    int want = rows < 4002 ? 4002 : rows + 2;
    float* nt = nullptr;
    HIP_TRY(hipMalloc(&nt, (size_t)want * kHidden * sizeof(float)));
    hipError_t err = launch_sinusoid_table(nt, want, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) {
        (void)hipFree(nt);
        return fail(LOCO_E_HIP, "sinusoid table: %s", hipGetErrorString(err));
    }
    if (float* old = e->sin_tab.load(std::memory_order_relaxed)) e->retired.push_back(old);
    e->sin_tab.store(nt, std::memory_order_release);
    e->sin_rows.store(want, std::memory_order_release);
    *tab = nt;
    e->sin_user = false;
    return LOCO_OK;
}

}  // namespace loco::host

namespace {

struct Bufs {
    int32_t* frames;
    const int32_t* frames_or_null;
    float *bufA, *bufB, *x0, *x1, *tmp, *ctx, *qkv, *qp, *ffn;
    _Float16 *xs0, *xs1;
    char* c0scratch;
    // packed forward (null otherwise): per clip, the conv-layer-0 frame count and the encoder frame count of its own reference batch
    const int32_t* t0_clip = nullptr;
    const int32_t* rows_clip = nullptr;
    const float* sin_tab = nullptr;  // the sinusoid table this forward reads (a snapshot: ensure_sin_rows)
};

// The start of every (half-)batch: its buffers at the plan's offsets in its workspace (frames_or_null, which depends on the mask,
// is the caller's), its split-K workspace, and its walk of the range slots from slot 0.
Bufs carve_bufs(Call& c, const Plan& p, char* ws, int32_t* out_frames) {
    auto f32 = [ws](size_t off) { return reinterpret_cast<float*>(ws + off); };
    c.splitk = p.splitk ? f32(p.off_splitk) : nullptr;
    c.nslot = 0;
    return {out_frames ? out_frames : reinterpret_cast<int32_t*>(ws + p.off_frames), nullptr, f32(p.off_a), f32(p.off_b), f32(p.off_x0),
            f32(p.off_x1), f32(p.off_tmp), f32(p.off_ctx), f32(p.off_qkv), f32(p.off_qp), f32(p.off_ffn),
            reinterpret_cast<_Float16*>(ws + p.off_xs0), reinterpret_cast<_Float16*>(ws + p.off_xs1), ws + p.off_c0scratch};
}

// conv layer 0 + GroupNorm + GELU (HF :484-494) of one (half-)batch: fp32 y, or the planes yhi / ylo
int run_conv0(loco_encoder* e, hipStream_t s, const Plan& p, const float* wav, const Bufs& bf, float* y, _Float16* yhi, _Float16* ylo,
              float* range_slot) {
    const double outb = 4.0 * p.B * (double)p.Tc[0] * kConvDim;
    Bracket br(e, s, K_CONV0, 2.0 * 10 * p.B * (double)p.Tc[0] * kConvDim, outb + 8.0 * p.B * (double)p.L);
    HIP_TRY(launch_conv0_gn_gelu(wav, p.B, p.L, e->conv_w[0], e->stem.conv0_norm.w, e->stem.conv0_norm.b, y, bf.c0scratch, e->cfg.ln_eps, s,
                                 yhi, ylo, range_slot, bf.t0_clip));
    return LOCO_OK;
}

// a fp32 buffer of n elements holds the two fp16 planes of n elements back to back
void planes(float* base, size_t n, _Float16*& hi, _Float16*& lo) {
    hi = reinterpret_cast<_Float16*>(base);
    lo = hi + n;
}

// ---- precision 0: every contraction on the exact-fp32 MFMA ------------------------------------------------------
// prenet: waveform -> x0, the encoder's input hidden states
int prenet_f32(loco_encoder* e, const Plan& p, const float* wav, const Bufs& bf, hipStream_t s) {
    const int B = p.B;
    const long M = p.M;
    const StemW& sw = e->stem;
    // ---- feature encoder (HF :484-494)
    LOCO_TRY(run_conv0(e, s, p, wav, bf, bf.bufA, nullptr, nullptr, nullptr));
    float* cin = bf.bufA;
    float* cout = bf.bufB;
    for (int i = 1; i < 7; ++i) {
        const long Tin = p.Tc[i - 1], Tout = p.Tc[i];
        LOCO_TRY(run_gemm(e, s, cin, (long)kConvS[i] * kConvDim, e->conv_w[i], (long)kConvK[i] * kConvDim, nullptr, nullptr, 0,
                          cout, kConvDim, (int)Tout, kConvDim, kConvK[i] * kConvDim, kEpiGelu, B, 1, Tin * kConvDim, 0,
                          Tout * kConvDim, 0));
        std::swap(cin, cout);
    }
    float* feats = cin;  // [M,512]
    if (e->tap_conv) LOCO_TRY(run_copy(e, s, e->tap_conv, feats, (size_t)M * kConvDim));

    // ---- feature projection (HF :498-510): LayerNorm(512) in place, then Linear(512,768)
    LOCO_TRY(run_ln(e, s, feats, sw.proj_norm.w, sw.proj_norm.b, feats, M, kConvDim));
    LOCO_TRY(run_gemm(e, s, feats, kConvDim, sw.proj.w, kConvDim, sw.proj.b, nullptr, 0, bf.x1, kHidden, (int)M, kHidden, kConvDim,
                      kEpiNone));
    if (e->tap_proj) LOCO_TRY(run_copy(e, s, e->tap_proj, bf.x1, (size_t)M * kHidden));

    // ---- positional conv + sinusoid (HF :555-564)
    {
        Bracket br(e, s, K_POSCONV, 2.0 * M * (double)kHidden * kPosCg * kPosK, 8.0 * M * kHidden);
        HIP_TRY(launch_pos_conv(bf.x1, e->pos_w, sw.pos_b, bf.sin_tab, bf.frames_or_null, bf.x0, B, (int)p.T, s, bf.rows_clip));
    }
    if (e->tap_prenet) LOCO_TRY(run_copy(e, s, e->tap_prenet, bf.x0, (size_t)M * kHidden));
    return LOCO_OK;
}

// output_attentions: layer l's probabilities into the bound buffer, right after the layer's attention launch (nothing when unbound).
// The f16 planes use all three MFMA terms in every plane mode, as the attention kernel does for its own QK^T.
int run_attention_probs(loco_encoder* e, hipStream_t s, const float* qkv, const _Float16* qhi, const _Float16* qlo, const _Float16* khi,
                        const _Float16* klo, const float* qp, const int32_t* frames, int l, int B, int T) {
    if (e->attn_probs.empty()) return LOCO_OK;
    const double tt = (double)B * kHeads * T * (double)T;
    Bracket br(e, s, K_ATTN_PROBS, 2.0 * 2.0 * tt * kHeadDim, 4.0 * tt);
    HIP_TRY(launch_attention_probs(qkv, qhi, qlo, khi, klo, qp, frames, e->attn_probs[l], B, T, 3, s));
    return LOCO_OK;
}

// encoder (HF :1276-1304): x0 -> out, and the hidden states the caller asked for
int encoder_f32(loco_encoder* e, const Plan& p, float* out, float* const* hidden_states, const Bufs& bf, hipStream_t s) {
    const int B = p.B;
    const int T = (int)p.T;
    const long M = p.M;
    float *x0 = bf.x0, *x1 = bf.x1, *tmp = bf.tmp, *ctx = bf.ctx, *qkv = bf.qkv, *qp = bf.qp, *ffn = bf.ffn;
    LOCO_TRY(run_ln(e, s, x0, e->stem.layer_norm.w, e->stem.layer_norm.b, x0, M, kHidden));
    const int nl = e->cfg.layers;
    for (int l = 0; l < nl; ++l) {
        if (hidden_states && hidden_states[l]) LOCO_TRY(run_copy(e, s, hidden_states[l], x0, (size_t)M * kHidden));
        const LayerW& lw = e->layers[l];
        // fused q|k|v projection, q pre-scaled (HF :891,911-914)
        LOCO_TRY(run_gemm(e, s, x0, kHidden, lw.wqkv, kHidden, lw.bqkv, nullptr, 0, qkv, kQkv, (int)M, kQkv, kHidden, kEpiNone));
        // Qp[b,h] = q_scaled[b,:,h,:] pe_k^T  -> [B,12,T,320]
        LOCO_TRY(run_gemm(e, s, qkv, kQkv, e->stem.pe_k, kHeadDim, nullptr, nullptr, 0, qp, kRelN, T, kRelN, kHeadDim, kEpiNone, B,
                          kHeads, (long)T * kQkv, kHeadDim, (long)kHeads * T * kRelN, (long)T * kRelN));
        {
            const double tt = (double)T * T;
            Bracket br(e, s, K_ATTN, 4.0 * B * kHeads * tt * kHeadDim, 4.0 * (M * (double)(kQkv + kHidden) + M * (double)kHeads * kRelN));
            HIP_TRY(launch_attention(qkv, qp, bf.frames_or_null, ctx, B, T, s));
        }
        LOCO_TRY(run_attention_probs(e, s, qkv, nullptr, nullptr, nullptr, nullptr, qp, bf.frames_or_null, l, B, T));
        // out_proj + residual (HF :984,1056), LayerNorm (HF :1058)
        LOCO_TRY(run_gemm(e, s, ctx, kHidden, lw.out_proj.w, kHidden, lw.out_proj.b, x0, kHidden, tmp, kHidden, (int)M, kHidden, kHidden,
                          kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.layer_norm.w, lw.layer_norm.b, x1, M, kHidden));
        // FFN (HF :1003-1010) + residual + final LayerNorm (HF :1059-1060)
        LOCO_TRY(run_gemm(e, s, x1, kHidden, lw.ffn_in.w, kHidden, lw.ffn_in.b, nullptr, 0, ffn, e->cfg.ffn, (int)M, e->cfg.ffn, kHidden,
                          kEpiGelu));
        LOCO_TRY(run_gemm(e, s, ffn, e->cfg.ffn, lw.ffn_out.w, e->cfg.ffn, lw.ffn_out.b, x1, kHidden, tmp, kHidden, (int)M, kHidden,
                          e->cfg.ffn, kEpiResidual));
        float* dst = (l == nl - 1) ? out : x0;
        LOCO_TRY(run_ln(e, s, tmp, lw.final_layer_norm.w, lw.final_layer_norm.b, dst, M, kHidden));
    }
    if (nl == 0) LOCO_TRY(run_copy(e, s, out, x0, (size_t)M * kHidden));
    if (hidden_states && hidden_states[nl]) LOCO_TRY(run_copy(e, s, hidden_states[nl], out, (size_t)M * kHidden));
    return LOCO_OK;
}

// ---- precision 1: every contraction (conv layers 1-6, feature projection, positional conv, QKV / out / FFN projections, the
// Qp table, QK^T and PV) on the fp16 x3 split MFMA; every producer writes the fp16 hi/lo planes its consumer needs, so no
// separate conversion pass exists.  conv0 (10 taps, VALU), residuals, GroupNorm / LayerNorm statistics and softmax stay fp32.
int prenet_f16x3(loco_encoder* e, Call& c, const Plan& p, const float* wav, const Bufs& bf, hipStream_t s) {
    const int B = p.B;
    const int T = (int)p.T;
    const long M = p.M;
    const StemW& sw = e->stem;
    static const char* const kConvNames[7] = {"feature_encoder.conv_layers.0 (GroupNorm + GELU)", "feature_encoder.conv_layers.1",
                                              "feature_encoder.conv_layers.2", "feature_encoder.conv_layers.3",
                                              "feature_encoder.conv_layers.4", "feature_encoder.conv_layers.5",
                                              "feature_encoder.conv_layers.6"};
    // ---- feature encoder: conv0 writes planes, conv1-5 planes -> planes, conv6 planes -> fp32 (LayerNorm input)
    _Float16 *ihi, *ilo, *ohi, *olo;
    planes(bf.bufA, (size_t)B * p.Tc[0] * kConvDim, ihi, ilo);
    LOCO_TRY(run_conv0(e, s, p, wav, bf, nullptr, ihi, ilo, c.slot(kConvNames[0])));
    float* cin = bf.bufA;
    float* cout = bf.bufB;
    for (int i = 1; i < 7; ++i) {
        const long Tin = p.Tc[i - 1], Tout = p.Tc[i];
        planes(cin, (size_t)B * Tin * kConvDim, ihi, ilo);
        planes(cout, (size_t)B * Tout * kConvDim, ohi, olo);
        GemmSplitArgs a = split_args(Tout, kConvDim, kConvK[i] * kConvDim, kEpiGelu);
        a.Ahi = ihi; a.Alo = ilo; a.lda = (long)kConvS[i] * kConvDim; a.ktaps = kConvK[i];
        a.nb1 = B; a.sA1 = Tin * kConvDim; a.sC1 = Tout * kConvDim;
        if (i == 6) {
            a.C = cout;
        } else {
            a.Chi = ohi; a.Clo = olo;
            a.range_slot = c.slot(kConvNames[i]);
        }
        LOCO_TRY(run_gemm_split(e, c, s, a, e->conv_s[i]));
        std::swap(cin, cout);
    }
    float* feats = cin;  // [M,512] fp32
    if (e->tap_conv) LOCO_TRY(run_copy(e, s, e->tap_conv, feats, (size_t)M * kConvDim));

    // ---- feature projection: LayerNorm(512) -> planes (in the idle conv buffer) -> Linear(512,768) -> x1 fp32
    planes(cout, (size_t)M * kConvDim, ohi, olo);
    LOCO_TRY(run_ln(e, s, feats, sw.proj_norm.w, sw.proj_norm.b, nullptr, M, kConvDim, ohi, olo));
    GemmSplitArgs a = split_args(M, kHidden, kConvDim, kEpiNone);
    a.Ahi = ohi; a.Alo = olo; a.bias = sw.proj.b; a.C = bf.x1;
    LOCO_TRY(run_gemm_split(e, c, s, a, e->proj_s));
    if (e->tap_proj) LOCO_TRY(run_copy(e, s, e->tap_proj, bf.x1, (size_t)M * kHidden));

    // ---- positional conv + sinusoid as ONE split GEMM per (clip, group): x1 is re-laid group-major with a 64-frame zero
    // halo, so that output frame t reads the contiguous run of 128 taps x 48 channels (lda = 48, K = 6144); the epilogue
    // fuses bias, GELU, the residual x1 and the sinusoidal-position gather (HF :389-397,555-564)
    _Float16* ghi = reinterpret_cast<_Float16*>(bf.ffn);  // scratch: the FFN buffer is idle until the first layer
    _Float16* glo = ghi + (size_t)B * kPosGroups * (T + kPosK) * kPosCg;
    {
        Bracket br(e, s, K_COPY, 0.0, 8.0 * M * kHidden);
        HIP_TRY(launch_group_major_split(bf.x1, ghi, glo, B, T, s, c.slot("feature_projection (input of pos_conv_embed)"), bf.rows_clip));
    }
    a = split_args(T, kPosCg, kPosK * kPosCg, kEpiPosConv);
    a.Ahi = ghi; a.Alo = glo; a.bias = sw.pos_b; a.R = bf.x1; a.C = bf.x0;
    a.lda = kPosCg; a.ldc = kHidden; a.ldr = kHidden;
    a.nb1 = B; a.nb2 = kPosGroups;
    a.sA1 = (long)kPosGroups * (T + kPosK) * kPosCg; a.sA2 = (long)(T + kPosK) * kPosCg;
    a.sC1 = (long)T * kHidden; a.sC2 = kPosCg;
    a.sW2 = (long)kPosCg * kPosK * kPosCg; a.sBias2 = kPosCg;
    a.sin_table = bf.sin_tab; a.frames = bf.frames_or_null; a.T = T;
    LOCO_TRY(run_gemm_split(e, c, s, a, e->posg_s, K_POSCONV_SPLIT, 2.0 * M * (double)kHidden * kPosCg * kPosK, 8.0 * M * kHidden));
    if (e->tap_prenet) LOCO_TRY(run_copy(e, s, e->tap_prenet, bf.x0, (size_t)M * kHidden));
    return LOCO_OK;
}

int encoder_f16x3(loco_encoder* e, Call& c, const Plan& p, float* out, float* const* hidden_states, const Bufs& bf, hipStream_t s) {
    const int B = p.B;
    const int T = (int)p.T;
    const long M = p.M;
    const int F = e->cfg.ffn;
    const size_t MH = (size_t)M * kHidden;
    float *x0 = bf.x0, *tmp = bf.tmp;
    // q / k / v as fp16 hi|lo planes [M,768] carved from the qkv region (attention clamps the key rows of its last tile to T - 1
    // and multiplies them by P = 0: nothing to pad or to zero)
    _Float16* qshi = reinterpret_cast<_Float16*>(bf.qkv);
    _Float16* qslo = qshi + MH;
    // planes in the order q_hi, q_lo, k_hi, k_lo, v_hi, v_lo: the k and v pairs sit 2 M 768 halves behind the pair before them
    _Float16* const kshi = qslo + MH;
    _Float16* const kslo = kshi + MH;
    _Float16* const vshi = kslo + MH;
    _Float16* const vslo = vshi + MH;
    _Float16 *x0hi = bf.xs0, *x0lo = bf.xs0 + MH;
    _Float16 *x1hi = bf.xs1, *x1lo = bf.xs1 + MH;
    _Float16 *chi, *clo, *fhi, *flo;
    planes(bf.ctx, MH, chi, clo);
    planes(bf.ffn, (size_t)M * F, fhi, flo);
    // Between layers the residual stream exists only as its fp16 hi/lo planes (22 bits): they are what the next GEMM reads
    // as its A operand anyway, and the residual adds reconstruct hi + lo exactly.  An fp32 copy is written only where
    // somebody reads one: hidden-state outputs, the zero-layer configuration, and the final output.
    const int nl = e->cfg.layers;
    float* x0f = (hidden_states || nl == 0) ? x0 : nullptr;
    LOCO_TRY(run_ln(e, s, x0, e->stem.layer_norm.w, e->stem.layer_norm.b, x0f, M, kHidden, x0hi, x0lo));
    for (int l = 0; l < nl; ++l) {
        if (hidden_states && hidden_states[l]) LOCO_TRY(run_copy(e, s, hidden_states[l], x0, MH));
        const LayerW& lw = e->layers[l];
        // fused q|k|v projection -> q, k and v as fp16 hi/lo planes [M,768] (the layout attention_f16x3 reads; it transposes V itself)
        GemmSplitArgs a = split_args(M, kQkv, kHidden, kEpiQkvScatter);
        a.Ahi = x0hi; a.Alo = x0lo; a.bias = lw.bqkv;
        a.Chi = qshi; a.Clo = qslo; a.ldc = kHidden; a.qkv_stride = (long)2 * M * kHidden; a.T = T;
        a.range_slot = c.slot("attention q|k|v projections", l);
        LOCO_TRY(run_gemm_split(e, c, s, a, lw.sqkv));
        dbg_planes(e, s, "x0 planes %s (layer input)", l, x0hi, x0lo, MH, kHidden);
        dbg_planes(e, s, "q planes %s", l, qshi, qslo, MH, kHidden);
        dbg_planes(e, s, "k planes %s", l, kshi, kslo, MH, kHidden);
        dbg_planes(e, s, "v planes %s", l, vshi, vslo, MH, kHidden);
        // Qp[b,h] = q_scaled[b,:,h,:] pe_k^T -> fp32 [B,12,T,320] is computed INSIDE the attention kernel (attention_f16x3.hip,
        // TABLE form): `qp` is scratch of that launch; no table GEMM runs any more.
        {
            const double tt = (double)T * T;
            // algorithmic FLOPs: QK^T + PV (4 T^2 64 per head) + the compact relative-position table (2 T 320 64 per head);
            // algorithmic bytes: q|k|v in, context out -- the table is now an internal scratch of the launch, not compulsory traffic
            Bracket br(e, s, K_ATTN_SPLIT, 4.0 * B * kHeads * tt * kHeadDim + 2.0 * M * (double)kHeads * kRelN * kHeadDim,
                       4.0 * (M * (double)(kQkv + kHidden)));
            HIP_TRY(launch_attention_f16x3(qshi, qslo, kshi, kslo, vshi, vslo, bf.qp, bf.frames_or_null, chi, clo, nullptr, B, T,
                                           s, e->pe_s.hi, e->pe_s.lo, e->pe_s.inv_scale));
        }
        // bf.qp now holds the blocks that launch formed, and stale workspace everywhere else -- whole rows of it where every valid key is
        // past-clipped.  The probabilities kernel reads only formed entries: rows i >= frames + 158 read none (include/loco_asr.h)
        LOCO_TRY(run_attention_probs(e, s, nullptr, qshi, qslo, kshi, kslo, bf.qp, bf.frames_or_null, l, B, T));
        dbg_planes(e, s, "attention context planes %s", l, chi, clo, MH, kHidden);
        // out_proj, then residual + LayerNorm: the GEMM stores acc + bias and the LayerNorm behind it adds x0 = hi + lo while it
        // streams the row -- the two additions of the residual epilogue in the same order (the same bits), without twelve waves
        // that hold the CU's LDS waiting for the planes in front of every store
        a = split_args(M, kHidden, kHidden, kEpiNone);
        a.Ahi = chi; a.Alo = clo; a.bias = lw.out_proj.b; a.C = tmp;
        LOCO_TRY(run_gemm_split(e, c, s, a, lw.so));
        dbg_check(e, s, "out_proj (fp32, before the residual)", l, tmp, MH, false, kHidden);
        LOCO_TRY(run_ln(e, s, tmp, lw.layer_norm.w, lw.layer_norm.b, nullptr, M, kHidden, x1hi, x1lo, nullptr, x0hi, x0lo));
        dbg_planes(e, s, "layer_norm planes %s", l, x1hi, x1lo, MH, kHidden);
        // FFN, then residual + final LayerNorm (the residual x1 joins in the LayerNorm, as above)
        a = split_args(M, F, kHidden, kEpiGelu);
        a.Ahi = x1hi; a.Alo = x1lo; a.bias = lw.ffn_in.b;
        a.Chi = fhi; a.Clo = flo; a.range_slot = c.slot("feed_forward intermediate (GELU)", l);
        LOCO_TRY(run_gemm_split(e, c, s, a, lw.s1));
        dbg_planes(e, s, "feed_forward intermediate planes %s", l, fhi, flo, (size_t)M * F, F);
        a = split_args(M, kHidden, F, kEpiNone);
        a.Ahi = fhi; a.Alo = flo; a.bias = lw.ffn_out.b; a.C = tmp;
        LOCO_TRY(run_gemm_split(e, c, s, a, lw.s2));
        dbg_check(e, s, "feed_forward output (fp32, before the residual)", l, tmp, MH, false, kHidden);
        const bool last = l == nl - 1;
        LOCO_TRY(run_ln(e, s, tmp, lw.final_layer_norm.w, lw.final_layer_norm.b, last ? out : (hidden_states ? x0 : nullptr), M, kHidden,
                        last ? nullptr : x0hi, last ? nullptr : x0lo,
                        last && c.range_dev ? c.range_dev + (size_t)kRangeShards * kFiniteStage : nullptr, x1hi, x1lo));
    }
    if (nl == 0) LOCO_TRY(run_copy(e, s, out, x0, MH));
    if (hidden_states && hidden_states[nl]) LOCO_TRY(run_copy(e, s, hidden_states[nl], out, MH));
    if (c.st) c.st->used = c.nslot;
    return LOCO_OK;
}

// the encoder stack of the call's precision family, on the x0 a prenet (speech or text) wrote
int encoder_stack(loco_encoder* e, Call& c, const Plan& p, float* out, float* const* hidden_states, const Bufs& bf, hipStream_t s) {
    return c.precision >= 1 ? encoder_f16x3(e, c, p, out, hidden_states, bf, s) : encoder_f32(e, p, out, hidden_states, bf, s);
}

// The status words travel to pinned host memory behind the forward, on its stream: readable once the stream has got there.
int range_begin(loco_encoder* e, Call& c, hipStream_t s) {
    StatusBlock* st = c.st;
    st->magic = kStatusMagic;
    st->precision = c.precision;
    st->used = 0;
    st->msg[0] = 0;
    if (c.precision >= 1 && !e->range_static.empty()) snprintf(st->msg, sizeof st->msg, "%s", e->range_static.c_str());
    if (c.precision >= 1) HIP_TRY(hipMemsetAsync(c.range_dev, 0, sizeof(float) * kRangeMaxStages * kRangeShards, s));
    return LOCO_OK;
}
int range_end(const Call& c, hipStream_t s) {
    if (c.precision >= 1 && c.st->used > 0)  // all of them (3 KiB): the tracked stages and the reserved finite-check word
        HIP_TRY(hipMemcpyAsync(c.st->words, c.range_dev, sizeof(float) * kRangeShards * kRangeMaxStages, hipMemcpyDeviceToHost, s));
    return LOCO_OK;
}

// The enqueue of every forward around its body half(c, part, ws, stream), which enqueues one (half-)batch from its workspace
// `ws`: part 0 is the whole batch on the caller's stream or, with `dual`, its first half; part 1 is the second half on the side
// stream.  Here: the Call, the status block's range words, and the fork and join of the side stream.
template <class Half>
int enqueue(loco_encoder* e, int precision, StatusBlock* st, void* workspace, hipStream_t s, bool dual, const Half& half) {
    Call c;
    c.precision = precision;
    c.st = st;
    c.range_dev = reinterpret_cast<float*>(workspace);
    char* ws = reinterpret_cast<char*>(workspace) + kStatusDevBytes;
    int rc = range_begin(e, c, s);
    if (rc) return rc;
    if (!dual) {
        rc = half(c, 0, ws, s);
        return rc ? rc : range_end(c, s);
    }

    // The side stream is one per handle: forwards in flight together take turns on it (the lock covers the enqueue only).
    std::lock_guard<std::mutex> lock(e->side_mu);
    if (!e->side) {
        HIP_TRY(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(e->ev_fork, s));  // the side stream starts after everything already queued on the caller's stream
    HIP_TRY(hipStreamWaitEvent(e->side, e->ev_fork, 0));
    // From here on the side stream may hold work that reads the caller's buffers and the workspace: whatever fails below, the
    // caller's stream is joined to it before this function returns, so that "stream idle" still means "workspace free".
    c.dual = true;
    rc = half(c, 0, ws, s);
    if (!rc) rc = half(c, 1, ws, e->side);  // it walks the same range slots as the first half (carve_bufs)
    c.dual = false;
    // a failed half has set loco_last_error; nothing below overwrites it
    const hipError_t j1 = hipEventRecord(e->ev_join, e->side);  // ... and the caller's stream continues after both halves
    const hipError_t j2 = j1 == hipSuccess ? hipStreamWaitEvent(s, e->ev_join, 0) : j1;
    if (j2 != hipSuccess) {
        // the join itself failed: block until the side stream has drained rather than hand back a workspace in use
        (void)hipStreamSynchronize(e->side);
        if (!rc) return fail(LOCO_E_HIP, "loco_forward: joining the second stream failed: %s", hipGetErrorString(j2));
    }
    return rc ? rc : range_end(c, s);
}

// What the loco_forward*_async entries share around run(mode, st): the precision and the status block are checked, and the
// block is no valid status until the enqueue has succeeded.
template <class Run>
int with_status(const loco_encoder* e, const char* fn, int precision, void* status, const Run& run) {
    if (precision != -1 && !loco_precision_name(precision))
        return fail(LOCO_E_INVALID, "%s: precision must be -1 (the handle's mode) or one of " LOCO_PRECISION_MODES, fn);
    if (reinterpret_cast<uintptr_t>(status) & 7) return fail(LOCO_E_INVALID, "%s: the status block must be 8-byte aligned", fn);
    StatusBlock* st = reinterpret_cast<StatusBlock*>(status);
    st->magic = 0;  // not a valid status until the enqueue has succeeded
    const int rc = run(precision < 0 ? e->precision : precision, st);
    if (rc) st->magic = 0;
    return rc;
}

// Two half-batches on two streams: clips are independent, so the halves give the same bits as one pass, and the tail of
// every kernel of one half (the last, partly filled round of workgroups: up to 12 % of the N = 768 GEMMs) is filled by
// the other half's kernels.  Measured gain (tools/two_stream_probe.py): +2 % at 32 x 30 s, +5..8 % at 16-32 clips of 2.5-15 s;
// halves of fewer than ~1000 frames (8 x 5 s) lose 4 %, so those stay on one stream.
bool split_batch(const loco_encoder* e, int B, long L, Plan& p0, Plan& p1) {
    if (e->streams < 2 || B < 2) return false;
    const int B0 = (B + 1) / 2;
    if (!make_plan(e, B0, L, p0) || !make_plan(e, B - B0, L, p1)) return false;
    return p1.M >= 1024;
}

// One (half-)batch of a speech forward: frame counts, the packed forward's clip tables, prenet and encoder stack.
// clip_t0 / clip_rows / clip_valid: null, or (loco_forward_packed) the host tables of THIS (half-)batch's clips
int forward_speech(loco_encoder* e, Call& c, const Plan& p, const float* wav, const int32_t* mask, float* out, int32_t* out_frames,
                   float* const* hidden_states, char* ws, hipStream_t s, const int32_t* clip_t0, const int32_t* clip_rows,
                   const int32_t* clip_valid, const float* sin_tab) {
    const int B = p.B;
    Bufs bf = carve_bufs(c, p, ws, out_frames);
    // ---- valid frame counts (HF :569-598); a packed forward that was given valid_len has them from the host (below)
    if (!clip_valid) {
        Bracket br(e, s, K_FRAMES, 0.0, mask ? 4.0 * B * (double)p.L : 0.0);
        HIP_TRY(launch_frame_counts(mask, B, p.L, bf.frames, s));
    }
    bf.frames_or_null = mask ? bf.frames : nullptr;
    bf.sin_tab = sin_tab;
    if (clip_t0) {
        // packed forward: the per-clip tables follow the stream into the workspace; without a mask every sample of a clip's own
        // reference batch counts, so its valid frames are that batch's frames (and a key mask is needed whatever the caller passed:
        // clips of shorter batches end before the pack does)
        int32_t* tab = reinterpret_cast<int32_t*>(ws + p.off_clip);
        HIP_TRY(hipMemcpyAsync(tab, clip_t0, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(tab + B, clip_rows, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (clip_valid) HIP_TRY(hipMemcpyAsync(bf.frames, clip_valid, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
        else if (!mask) HIP_TRY(hipMemcpyAsync(bf.frames, tab + B, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        bf.frames_or_null = bf.frames;
        bf.t0_clip = tab;
        bf.rows_clip = tab + B;
    }
    const int rc = c.precision >= 1 ? prenet_f16x3(e, c, p, wav, bf, s) : prenet_f32(e, p, wav, bf, s);
    return rc ? rc : encoder_stack(e, c, p, out, hidden_states, bf, s);
}

// One forward in arithmetic mode `precision`, its range words in the first bytes of the workspace, its status in `st`.  Nothing
// the enqueue mutates is shared between calls except the lazily created side stream (side_mu), the profiling records (profiling
// is a single-caller diagnostic mode) and the sinusoid table when a clip longer than any before makes it grow.
int forward_impl(loco_encoder* e, int precision, StatusBlock* st, const float* wav, const int32_t* mask, int32_t B, int64_t L, float* out,
                 int32_t* out_frames, float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream,
                 const int64_t* pad_len = nullptr, const int64_t* valid_len = nullptr) {
    if (!e || !wav || !out || !workspace || !st) return fail(LOCO_E_INVALID, "loco_forward: null argument");
    if (!e->finalized) return fail(LOCO_E_STATE, "loco_forward: call loco_finalize_weights first");
    if (!e->speech_ready) return fail(LOCO_E_STATE, "loco_forward: this encoder was loaded without the speech prenet weights");
    Plan p, p0, p1;
    if (!make_plan(e, B, L, p))
        return fail(LOCO_E_INVALID, "loco_forward: batch %d x %lld samples gives no output frame (need >= 400 samples)", B, (long long)L);
    if (B > 65535) return fail(LOCO_E_INVALID, "loco_forward: batch %d > 65535", B);
    if (p.M > 0x7fffffffL / 8) return fail(LOCO_E_INVALID, "loco_forward: B*T = %ld frames is too large", p.M);
    // per-kernel timing, hidden-state, tap and attention outputs keep the single in-order pass
    const bool dual = !e->profiling && !hidden_states && !e->tap_conv && !e->tap_proj && !e->tap_prenet && e->attn_probs.empty() &&
                      split_batch(e, B, L, p0, p1);
    const size_t need = kStatusDevBytes + (dual ? p0.total + p1.total : p.total);
    if (workspace_bytes < need)
        return fail(LOCO_E_WORKSPACE, "loco_forward: workspace %zu < required %zu bytes", workspace_bytes, need);
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) || (reinterpret_cast<uintptr_t>(wav) & 3))
        return fail(LOCO_E_INVALID, "loco_forward: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const float* sin_tab = nullptr;  // this forward's snapshot of the sinusoid table
    int rc = ensure_sin_rows(e, (int)p.T + 2, s, &sin_tab);
    if (rc) return rc;
    const int32_t *tab_t0 = nullptr, *tab_rows = nullptr, *tab_valid = nullptr;
    if (pad_len) {  // loco_forward_packed: validate, then derive the two per-clip frame counts into the caller's status block
        if (B > kMaxPackClips) return fail(LOCO_E_INVALID, "loco_forward_packed: %d clips > %d", B, kMaxPackClips);
        for (int b = 0; b < B; ++b) {
            if (pad_len[b] > L || loco_output_frames(pad_len[b]) < 1)
                return fail(LOCO_E_INVALID, "loco_forward_packed: pad_len[%d] = %lld must lie in [400, L = %lld]", b, (long long)pad_len[b],
                            (long long)L);
            st->clip_tab[b] = (int32_t)conv_out_len(pad_len[b], kConvK[0], kConvS[0]);
            st->clip_tab[B + b] = (int32_t)loco_output_frames(pad_len[b]);
            if (valid_len) {
                if (valid_len[b] < 0 || valid_len[b] > pad_len[b])
                    return fail(LOCO_E_INVALID, "loco_forward_packed: valid_len[%d] = %lld must lie in [0, pad_len = %lld]", b,
                                (long long)valid_len[b], (long long)pad_len[b]);
                st->clip_tab[2 * B + b] = (int32_t)loco_output_frames(valid_len[b]);  // as frames_from_counts_kernel: HF's floor division
            }
        }
        tab_t0 = st->clip_tab;
        tab_rows = st->clip_tab + B;
        if (valid_len) tab_valid = st->clip_tab + 2 * B;
    }
    return enqueue(e, precision, st, workspace, s, dual, [&](Call& c, int part, char* ws, hipStream_t hs) {
        if (part == 0)
            return forward_speech(e, c, dual ? p0 : p, wav, mask, out, out_frames, hidden_states, ws, hs, tab_t0, tab_rows, tab_valid,
                                  sin_tab);
        const int B0 = p0.B;  // the second half starts B0 clips into every per-clip input and output
        auto skip = [B0](const int32_t* tab) { return tab ? tab + B0 : nullptr; };
        return forward_speech(e, c, p1, wav + (size_t)B0 * L, mask ? mask + (size_t)B0 * L : nullptr, out + (size_t)B0 * p.T * kHidden,
                              out_frames ? out_frames + B0 : nullptr, nullptr, ws + p0.total, hs, skip(tab_t0), skip(tab_rows),
                              skip(tab_valid), sin_tab);
    });
}

int forward_text_impl(loco_encoder* e, int precision, StatusBlock* st, const int32_t* input_ids, const int32_t* attention_mask, int32_t B, int32_t T,
                      float* out, int32_t* out_frames, float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !input_ids || !out || !workspace || !st) return fail(LOCO_E_INVALID, "loco_forward_text: null argument");
    if (!e->finalized) return fail(LOCO_E_STATE, "loco_forward_text: call loco_finalize_weights first");
    if (!e->text_embed || !e->text_alpha || !e->text_pe)
        return fail(LOCO_E_STATE, "loco_forward_text: this encoder was loaded without the text prenet weights");
    Plan p;
    if (!make_plan_tokens(e, B, T, p)) return fail(LOCO_E_INVALID, "loco_forward_text: batch %d x %d tokens is empty", B, T);
    if (B > 65535) return fail(LOCO_E_INVALID, "loco_forward_text: batch %d > 65535", B);
    if (T > e->text_pe_rows)
        return fail(LOCO_E_INVALID, "loco_forward_text: %d tokens exceed the positional table (%d rows: max_text_positions)", T,
                    e->text_pe_rows);
    if (workspace_bytes < kStatusDevBytes + p.total)
        return fail(LOCO_E_WORKSPACE, "loco_forward_text: workspace %zu < required %zu bytes", workspace_bytes, kStatusDevBytes + p.total);
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(LOCO_E_INVALID, "loco_forward_text: workspace must be 256-byte aligned");
    return enqueue(e, precision, st, workspace, (hipStream_t)stream, false, [&](Call& c, int, char* ws, hipStream_t s) {
        Bufs bf = carve_bufs(c, p, ws, out_frames);
        {
            Bracket br(e, s, K_FRAMES, 0.0, attention_mask ? 4.0 * B * (double)T : 0.0);
            HIP_TRY(launch_token_counts(attention_mask, B, T, bf.frames, s));
        }
        {   // embed_tokens + alpha * pe (HF SpeechT5TextEncoderPrenet.forward)
            Bracket br(e, s, K_COPY, 0.0, 12.0 * p.M * kHidden);
            HIP_TRY(launch_text_prenet(input_ids, e->text_embed, e->text_vocab, e->text_alpha, e->text_pe, B, T, bf.x0, s));
        }
        bf.frames_or_null = attention_mask ? bf.frames : nullptr;
        return encoder_stack(e, c, p, out, hidden_states, bf, s);
    });
}

}  // namespace

extern "C" {

int64_t loco_output_frames(int64_t n) {
    for (int i = 0; i < 7; ++i) {
        const int64_t d = n - kConvK[i];
        n = (d >= 0 ? d / kConvS[i] : -((-d + kConvS[i] - 1) / kConvS[i])) + 1;
    }
    return n;
}

size_t loco_workspace_bytes(const loco_encoder* e, int32_t B, int64_t L) {
    Plan p, p0, p1;
    if (!e || !make_plan(e, B, L, p)) return 0;
    if (split_batch(e, B, L, p0, p1)) return kStatusDevBytes + std::max(p.total, p0.total + p1.total);
    return kStatusDevBytes + p.total;
}

int loco_forward(loco_encoder* e, const float* wav, const int32_t* mask, int32_t B, int64_t L, float* out,
                 int32_t* out_frames, float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e) return fail(LOCO_E_INVALID, "loco_forward: null argument");
    return forward_impl(e, e->precision, e->own, wav, mask, B, L, out, out_frames, hidden_states, workspace, workspace_bytes, stream);
}

int loco_forward_async(loco_encoder* e, int precision, const float* wav, const int32_t* mask, int32_t B, int64_t L, float* out,
                       int32_t* out_frames, float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream,
                       void* status) {
    if (!e || !status) return fail(LOCO_E_INVALID, "loco_forward_async: null argument");
    if (!e->attn_probs.empty()) return fail(LOCO_E_STATE, "loco_forward_async: attention outputs are bound (loco_set_attention_outputs)");
    return with_status(e, "loco_forward_async", precision, status, [&](int mode, StatusBlock* st) {
        return forward_impl(e, mode, st, wav, mask, B, L, out, out_frames, hidden_states, workspace, workspace_bytes, stream);
    });
}

int loco_forward_packed(loco_encoder* e, int precision, const float* wav, const int32_t* mask, const int64_t* valid_len, int32_t B, int64_t L,
                        const int64_t* pad_len, float* out, int32_t* out_frames, float* const* hidden_states, void* workspace,
                        size_t workspace_bytes, void* stream, void* status) {
    if (!e || !status || !pad_len) return fail(LOCO_E_INVALID, "loco_forward_packed: null argument");
    if (!e->attn_probs.empty()) return fail(LOCO_E_STATE, "loco_forward_packed: attention outputs are bound (loco_set_attention_outputs)");
    if (mask && valid_len) return fail(LOCO_E_INVALID, "loco_forward_packed: give attention_mask or valid_len, not both");
    return with_status(e, "loco_forward_packed", precision, status, [&](int mode, StatusBlock* st) {
        return forward_impl(e, mode, st, wav, mask, B, L, out, out_frames, hidden_states, workspace, workspace_bytes, stream, pad_len,
                            valid_len);
    });
}

int loco_max_pack_clips(void) { return kMaxPackClips; }

int loco_forward_checked(loco_encoder* e, const float* wav, const int32_t* mask, int32_t B, int64_t L, float* out, int32_t* out_frames,
                         float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream, int32_t* used_fp32) {
    if (used_fp32) *used_fp32 = 0;
    int rc = loco_forward(e, wav, mask, B, L, out, out_frames, hidden_states, workspace, workspace_bytes, stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    rc = loco_forward_status(e, nullptr, 0);
    if (rc != LOCO_E_RANGE || e->range_policy == 0) return rc;
    // out of the fp16 planes' range: the same batch again on the exact-fp32 MFMA kernels of this library
    rc = forward_impl(e, 0, e->own, wav, mask, B, L, out, out_frames, hidden_states, workspace, workspace_bytes, stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (used_fp32) *used_fp32 = 1;
    return LOCO_OK;
}

// ---- text front end ---------------------------------------------------------------------------------------
size_t loco_text_workspace_bytes(const loco_encoder* e, int32_t B, int32_t T) {
    Plan p;
    if (!e || !make_plan_tokens(e, B, T, p)) return 0;
    return kStatusDevBytes + p.total;
}

int loco_text_max_positions(const loco_encoder* e) { return e ? e->text_pe_rows : 0; }

int loco_forward_text(loco_encoder* e, const int32_t* input_ids, const int32_t* attention_mask, int32_t B, int32_t T, float* out,
                      int32_t* out_frames, float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e) return fail(LOCO_E_INVALID, "loco_forward_text: null argument");
    return forward_text_impl(e, e->precision, e->own, input_ids, attention_mask, B, T, out, out_frames, hidden_states, workspace, workspace_bytes, stream);
}

int loco_forward_text_async(loco_encoder* e, int precision, const int32_t* input_ids, const int32_t* attention_mask, int32_t B, int32_t T,
                            float* out, int32_t* out_frames, float* const* hidden_states, void* workspace, size_t workspace_bytes,
                            void* stream, void* status) {
    if (!e || !status) return fail(LOCO_E_INVALID, "loco_forward_text_async: null argument");
    if (!e->attn_probs.empty())
        return fail(LOCO_E_STATE, "loco_forward_text_async: attention outputs are bound (loco_set_attention_outputs)");
    return with_status(e, "loco_forward_text_async", precision, status, [&](int mode, StatusBlock* st) {
        return forward_text_impl(e, mode, st, input_ids, attention_mask, B, T, out, out_frames, hidden_states, workspace, workspace_bytes,
                                 stream);
    });
}

}  // extern "C"
