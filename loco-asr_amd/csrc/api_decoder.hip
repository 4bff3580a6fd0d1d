// C ABI (include/loco_asr.h), the text decoder: teacher-forced logits, greedy generation, forced alignment, the slot pool with its
// sampling configuration, loco_decoder_score, and the decoder's attention, probability and DTW operators.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "loco_host.h"

using namespace loco;
using namespace loco::host;

// ---- text decoder: teacher-forced logits and greedy generation ------------------------------------------------------------
namespace {

// Workspace of one utterance batch (caller-owned): state that lives from loco_decoder_begin to the last step first, scratch after.
struct DecPlan {
    int B, T, S, L;
    size_t off_state, off_lengths, off_frames, off_tokens, off_nonpad, off_finished, off_cross, off_self, off_x0, off_x1, off_tmp, off_q,
        off_ctx, off_ffn, off_logits, off_attn, total;
};

void make_dec_plan(int layers, int B, int T, int S, DecPlan& p) {
    p.B = B, p.T = T, p.S = S, p.L = layers;
    const size_t f = sizeof(float), rows = (size_t)B * S;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o += align_up(bytes);
        return at;
    };
    p.off_state = take(4 * sizeof(int32_t));  // [0] rows still open, [1] steps completed
    p.off_lengths = take((size_t)B * sizeof(int32_t));
    p.off_frames = take((size_t)B * sizeof(int32_t));
    p.off_tokens = take(rows * sizeof(int32_t));
    p.off_nonpad = take(rows * sizeof(int32_t));
    p.off_finished = take(rows * sizeof(int32_t));
    p.off_cross = take((size_t)B * T * p.L * 2 * kHidden * f);  // [B * T_enc][layers][k | v]
    p.off_self = take((size_t)p.L * rows * 2 * kHidden * f);    // [layers][B][S_max][k | v]
    p.off_x0 = take(rows * kHidden * f);
    p.off_x1 = take(rows * kHidden * f);
    p.off_tmp = take(rows * kHidden * f);
    p.off_q = take(rows * kHidden * f);
    p.off_ctx = take(rows * kHidden * f);
    p.off_ffn = take(rows * kFfn * f);
    p.off_logits = take((size_t)B * 128 * f);
    size_t attn = dec_attention_scratch_bytes(B, S, T);  // teacher-forced cross-attention
    for (size_t v : {dec_attention_scratch_bytes(B, S, S), dec_attention_scratch_bytes(B, 1, T), dec_attention_scratch_bytes(B, 1, S)})
        attn = v > attn ? v : attn;
    p.off_attn = take(attn);
    p.total = o;
}

// what every decoder entry asks of its handle first (dec_check, pool_check)
int dec_handle_check(const loco_encoder* e, const char* fn) {
    if (!e) return fail(LOCO_E_INVALID, "%s: null encoder", fn);
    if (!e->finalized || !e->dec.ready)
        return fail(LOCO_E_STATE, "%s: the handle has no decoder weights (decoder.prenet.*, decoder.wrapped_decoder.*, text_decoder_postnet.*) or "
                                  "loco_finalize_weights has not run", fn);
    return LOCO_OK;
}

int dec_check(const loco_encoder* e, const char* fn, int B, int T, int S, const void* ws, size_t bytes, DecPlan& p) {
    LOCO_TRY(dec_handle_check(e, fn));
    if (B <= 0 || T <= 0 || S <= 0) return fail(LOCO_E_INVALID, "%s: B, T_enc and the sequence length must be positive", fn);
    if (S > kDecMaxPositions) return fail(LOCO_E_INVALID, "%s: %d positions exceed max_text_positions = %d", fn, S, kDecMaxPositions);
    if (!ws) return fail(LOCO_E_INVALID, "%s: null workspace", fn);
    make_dec_plan(e->dec.layers, B, T, S, p);
    if (bytes < p.total) return fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, bytes, p.total);
    return LOCO_OK;
}

int run_skinny(hipStream_t s, const float* A, const WB& w, const float* R, float* C, int M, int N, int K, int epi) {
    HIP_TRY(launch_skinny_gemm(A, K, w.w, K, w.b, R, N, C, N, nullptr, 0, N, M, N, K, epi, s));
    return LOCO_OK;
}

// cross-attention k|v of every layer from the encoder output: M = B * T_enc rows through the exact-fp32 GEMM (14 MFLOP per frame
// against the encoder's 339)
int dec_cross_kv(loco_encoder* e, const DecPlan& p, char* ws, const float* enc_out, hipStream_t s) {
    const int N = p.L * 2 * kHidden;
    return run_gemm(e, s, enc_out, kHidden, e->dec.wckv, kHidden, e->dec.bckv, nullptr, 0, reinterpret_cast<float*>(ws + p.off_cross), N,
                    p.B * p.T, N, kHidden, kEpiNone);
}

int dec_attention(hipStream_t s, const float* q, long ldq, long sq, const float* kv, long ldk, long sk, const int32_t* kcount, float* out,
                  int B, int Sq, int Tk, int causal, float* scratch) {
    HIP_TRY(launch_dec_attention(q, ldq, sq, kv, ldk, sk, kv + kHidden, ldk, sk, kcount, out, kHidden, (long)Sq * kHidden, B, Sq, Tk, causal, 0,
                                 1.0f, scratch, s));
    return LOCO_OK;
}

// one decode step: token t of every row in, token t + 1 out; B rows through the weight-streaming GEMM
int dec_step(loco_encoder* e, const DecPlan& p, char* ws, int t, float* logits_out, hipStream_t s) {
    const DecoderW& d = e->dec;
    const int B = p.B;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto I = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    float *x0 = F(p.off_x0), *x1 = F(p.off_x1), *tmp = F(p.off_tmp), *q = F(p.off_q), *ctx = F(p.off_ctx), *ffn = F(p.off_ffn), *scr = F(p.off_attn);
    float* logits = logits_out ? logits_out : F(p.off_logits);
    const long ld_cross = (long)p.L * 2 * kHidden, ld_self = 2 * kHidden;
    HIP_TRY(launch_dec_embed_step(I(p.off_tokens), p.S, t, d.embed, d.vocab, d.pos_tab, d.pos_rows, I(p.off_nonpad), x0, B, s));
    for (int l = 0; l < p.L; ++l) {
        const DecLayerW& lw = d.L[l];
        float* cache = F(p.off_self) + (size_t)l * B * p.S * ld_self;
        // q -> row buffer, k|v -> row t of the cache
        HIP_TRY(launch_skinny_gemm(x0, kHidden, lw.wqkv, kHidden, lw.bqkv, nullptr, 0, q, kHidden, cache + (size_t)t * ld_self, (long)p.S * ld_self,
                                   kHidden, B, kQkv, kHidden, kEpiNone, s));
        LOCO_TRY(dec_attention(s, q, kHidden, kHidden, cache, ld_self, (long)p.S * ld_self, nullptr, ctx, B, 1, t + 1, 0, scr));
        LOCO_TRY(run_skinny(s, ctx, lw.self_out, x0, tmp, B, kHidden, kHidden, kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.self_ln.w, lw.self_ln.b, x1, B, kHidden));
        LOCO_TRY(run_skinny(s, x1, WB{lw.wcq, lw.bcq}, nullptr, q, B, kHidden, kHidden, kEpiNone));
        LOCO_TRY(dec_attention(s, q, kHidden, kHidden, F(p.off_cross) + (size_t)l * 2 * kHidden, ld_cross, (long)p.T * ld_cross, I(p.off_frames), ctx, B,
                              1, p.T, 0, scr));
        LOCO_TRY(run_skinny(s, ctx, lw.cross_out, x1, tmp, B, kHidden, kHidden, kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.cross_ln.w, lw.cross_ln.b, x0, B, kHidden));
        LOCO_TRY(run_skinny(s, x0, lw.ffn_in, nullptr, ffn, B, kFfn, kHidden, kEpiGelu));
        LOCO_TRY(run_skinny(s, ffn, lw.ffn_out, x0, tmp, B, kHidden, kFfn, kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.final_ln.w, lw.final_ln.b, x0, B, kHidden));
    }
    LOCO_TRY(run_skinny(s, x0, WB{d.lm_head, nullptr}, nullptr, logits, B, d.vocab, kHidden, kEpiNone));
    HIP_TRY(launch_dec_select(logits, d.vocab, B, I(p.off_tokens), p.S, t, I(p.off_finished), I(p.off_lengths), I(p.off_state), kDecEosToken,
                              kDecPadToken, s));
    return LOCO_OK;
}

// the plan's key counts of the cross-attention: the caller's frame counts, or T_enc for every clip
int dec_set_frames(const DecPlan& p, char* ws, const int32_t* enc_frames, hipStream_t s) {
    int32_t* frames = reinterpret_cast<int32_t*>(ws + p.off_frames);
    if (enc_frames)
        HIP_TRY(hipMemcpyAsync(frames, enc_frames, (size_t)p.B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    else  // no frame counts: every encoder row is a key
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(frames), p.T, (size_t)p.B, s));
    return LOCO_OK;
}

int dec_begin(loco_encoder* e, const DecPlan& p, char* ws, const float* enc_out, const int32_t* enc_frames, hipStream_t s) {
    auto I = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    LOCO_TRY(dec_set_frames(p, ws, enc_frames, s));
    HIP_TRY(launch_dec_begin(I(p.off_tokens), p.B, p.S, kDecStartToken, kDecPadToken, I(p.off_lengths), I(p.off_state), s));
    return dec_cross_kv(e, p, ws, enc_out, s);
}

}  // namespace

int loco_decoder_max_batch(void) { return kSkinnyMaxM; }

size_t loco_decoder_workspace_bytes(const loco_encoder* e, int32_t B, int32_t T_enc, int32_t S_max) {
    if (!e || B <= 0 || T_enc <= 0 || S_max <= 0) return 0;
    if (!loco_has_decoder(e)) return 0;  // nothing to decode with
    DecPlan p;
    make_dec_plan(decoder_layers_loaded(e, nullptr), B, T_enc, S_max, p);  // the layers the loaded keys name
    return p.total;
}

namespace {

// What a teacher-forced pass hands out besides logits and hidden states.  All null: exactly loco_decoder_forward's launches.
struct DecAttnSink {
    float* const* self_attn = nullptr;   // host array of `layers` device pointers f32 [B,12,S,S], or null
    float* const* cross_attn = nullptr;  // ... f32 [B,12,S,T_enc], or null
    // loco_decoder_align: A = mean of the cross-attention P over the selected (layer, head) pairs, one layer's P in `scratch` at a time
    float* mean = nullptr;
    float* scratch = nullptr;
    const unsigned* heads = nullptr;  // [layers] bit h = head h of the layer is selected
    int pairs = 0, first_layer = 0, last_layer = 0;
};

// The layer walk of the teacher-forced pass, shared by loco_decoder_forward, loco_decoder_forward_attn and loco_decoder_align.  The
// probabilities are formed by launches of their own between the existing ones (each reads the q projection its attention launch read,
// before the next product overwrites it), so logits and hidden states are the same bits with and without them.  logits == null (the
// alignment): the walk ends after the last selected layer's cross-attention.
int dec_forward_walk(loco_encoder* e, const DecPlan& p, char* ws, const float* enc_out, const int32_t* enc_frames, const int32_t* decoder_input_ids,
                     float* logits, float* const* hidden_states, const DecAttnSink& sink, hipStream_t s) {
    const int B = p.B, T_enc = p.T, S = p.S;
    const DecoderW& d = e->dec;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto I = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    float *x0 = F(p.off_x0), *x1 = F(p.off_x1), *tmp = F(p.off_tmp), *q = F(p.off_q), *ctx = F(p.off_ctx), *ffn = F(p.off_ffn), *scr = F(p.off_attn);
    const int M = B * S;
    const long ld_cross = (long)p.L * 2 * kHidden, ld_self = 2 * kHidden;
    LOCO_TRY(dec_set_frames(p, ws, enc_frames, s));
    LOCO_TRY(dec_cross_kv(e, p, ws, enc_out, s));
    HIP_TRY(launch_dec_embed(decoder_input_ids, S, d.embed, d.vocab, d.pos_tab, d.pos_rows, x0, B, S, nullptr, s));
    for (int l = 0; l < p.L; ++l) {
        const DecLayerW& lw = d.L[l];
        if (hidden_states) LOCO_TRY(run_copy(e, s, hidden_states[l], x0, (size_t)M * kHidden));
        // the self-attention k|v land in the layout the step reads ([layers][B][S][k | v] with S rows per clip here)
        float* cache = F(p.off_self) + (size_t)l * M * ld_self;
        LOCO_TRY(run_gemm(e, s, x0, kHidden, lw.wqkv, kHidden, lw.bqkv, nullptr, 0, q, kHidden, M, kHidden, kHidden, kEpiNone));
        LOCO_TRY(run_gemm(e, s, x0, kHidden, lw.wqkv + (size_t)kHidden * kHidden, kHidden, lw.bqkv + kHidden, nullptr, 0, cache, ld_self, M, 2 * kHidden,
                         kHidden, kEpiNone));
        LOCO_TRY(dec_attention(s, q, kHidden, (long)S * kHidden, cache, ld_self, (long)S * ld_self, nullptr, ctx, B, S, S, 1, scr));
        if (sink.self_attn)
            HIP_TRY(launch_dec_attention_probs(q, kHidden, (long)S * kHidden, cache, ld_self, (long)S * ld_self, nullptr, sink.self_attn[l], B, S, S, 1,
                                               1.0f, s));
        LOCO_TRY(run_gemm(e, s, ctx, kHidden, lw.self_out.w, kHidden, lw.self_out.b, x0, kHidden, tmp, kHidden, M, kHidden, kHidden, kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.self_ln.w, lw.self_ln.b, x1, M, kHidden));
        LOCO_TRY(run_gemm(e, s, x1, kHidden, lw.wcq, kHidden, lw.bcq, nullptr, 0, q, kHidden, M, kHidden, kHidden, kEpiNone));
        const float* ck = F(p.off_cross) + (size_t)l * 2 * kHidden;
        LOCO_TRY(dec_attention(s, q, kHidden, (long)S * kHidden, ck, ld_cross, (long)T_enc * ld_cross, I(p.off_frames), ctx, B, S, T_enc, 0, scr));
        const bool averaged = sink.mean && sink.heads[l];
        float* pc = sink.cross_attn ? sink.cross_attn[l] : (averaged ? sink.scratch : nullptr);
        if (pc)
            HIP_TRY(launch_dec_attention_probs(q, kHidden, (long)S * kHidden, ck, ld_cross, (long)T_enc * ld_cross, I(p.off_frames), pc, B, S, T_enc, 0,
                                               1.0f, s));
        if (averaged)
            HIP_TRY(launch_dec_attn_mean(pc, sink.mean, B, S, T_enc, sink.heads[l], l == sink.first_layer, l == sink.last_layer,
                                         1.0f / (float)sink.pairs, s));
        if (!logits && !hidden_states && sink.mean && l == sink.last_layer) return LOCO_OK;
        LOCO_TRY(run_gemm(e, s, ctx, kHidden, lw.cross_out.w, kHidden, lw.cross_out.b, x1, kHidden, tmp, kHidden, M, kHidden, kHidden, kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.cross_ln.w, lw.cross_ln.b, x0, M, kHidden));
        LOCO_TRY(run_gemm(e, s, x0, kHidden, lw.ffn_in.w, kHidden, lw.ffn_in.b, nullptr, 0, ffn, kFfn, M, kFfn, kHidden, kEpiGelu));
        LOCO_TRY(run_gemm(e, s, ffn, kFfn, lw.ffn_out.w, kFfn, lw.ffn_out.b, x0, kHidden, tmp, kHidden, M, kHidden, kFfn, kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.final_ln.w, lw.final_ln.b, x0, M, kHidden));
    }
    if (hidden_states) LOCO_TRY(run_copy(e, s, hidden_states[p.L], x0, (size_t)M * kHidden));
    if (!logits) return LOCO_OK;
    // lm_head: N = vocab (81) is no multiple of the MFMA GEMM's 4-column epilogue; the weight-streaming kernel takes any N, 64 rows per grid row
    return run_skinny(s, x0, WB{d.lm_head, nullptr}, nullptr, logits, M, d.vocab, kHidden, kEpiNone);
}

int dec_forward_entry(const char* fn, loco_encoder* e, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc,
                      const int32_t* decoder_input_ids, int32_t S, float* logits, float* const* hidden_states, float* const* self_attentions,
                      float* const* cross_attentions, void* workspace, size_t workspace_bytes, void* stream) {
    DecPlan p;
    LOCO_TRY(dec_check(e, fn, B, T_enc, S, workspace, workspace_bytes, p));
    if (!enc_out || !decoder_input_ids || !logits) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    for (int l = 0; l < p.L; ++l)
        if ((self_attentions && !self_attentions[l]) || (cross_attentions && !cross_attentions[l]))
            return fail(LOCO_E_INVALID, "%s: null attention output of layer %d (an array of %d device pointers is expected)", fn, l, p.L);
    DecAttnSink sink;
    sink.self_attn = self_attentions, sink.cross_attn = cross_attentions;
    return dec_forward_walk(e, p, static_cast<char*>(workspace), enc_out, enc_frames, decoder_input_ids, logits, hidden_states, sink,
                            (hipStream_t)stream);
}

// loco_decoder_align's workspace: the decoder's own, then one layer's cross-attention P, A, the DTW's back-pointers
struct AlignPlan {
    DecPlan dec;
    size_t off_probs, off_mean, off_back, total;
};

void make_align_plan(int layers, int B, int T, int S, AlignPlan& a) {
    make_dec_plan(layers, B, T, S, a.dec);
    size_t o = a.dec.total;
    const size_t cells = (size_t)B * S * T;
    a.off_probs = o, o += align_up(cells * kHeads * sizeof(float));
    a.off_mean = o, o += align_up(cells * sizeof(float));
    a.off_back = o, o += align_up(cells);
    a.total = o;
}

}  // namespace

int loco_decoder_forward(loco_encoder* e, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc,
                         const int32_t* decoder_input_ids, int32_t S, float* logits, float* const* hidden_states, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return dec_forward_entry("loco_decoder_forward", e, enc_out, enc_frames, B, T_enc, decoder_input_ids, S, logits, hidden_states, nullptr, nullptr,
                             workspace, workspace_bytes, stream);
}

int loco_decoder_forward_attn(loco_encoder* e, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc,
                              const int32_t* decoder_input_ids, int32_t S, float* logits, float* const* hidden_states, float* const* self_attentions,
                              float* const* cross_attentions, void* workspace, size_t workspace_bytes, void* stream) {
    return dec_forward_entry("loco_decoder_forward_attn", e, enc_out, enc_frames, B, T_enc, decoder_input_ids, S, logits, hidden_states,
                             self_attentions, cross_attentions, workspace, workspace_bytes, stream);
}

size_t loco_decoder_align_workspace_bytes(const loco_encoder* e, int32_t B, int32_t T_enc, int32_t S) {
    if (!e || B <= 0 || T_enc <= 0 || S <= 0 || S > kDecMaxPositions) return 0;
    if (!loco_has_decoder(e)) return 0;
    AlignPlan a;
    make_align_plan(decoder_layers_loaded(e, nullptr), B, T_enc, S, a);
    return a.total;
}

int loco_decoder_align(loco_encoder* e, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc, const int32_t* decoder_input_ids,
                       int32_t S, const int32_t* token_counts, const int32_t* layer_heads, int32_t pairs, float* attention, int32_t* start_frames,
                       int32_t* end_frames, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "loco_decoder_align";
    DecPlan p;
    LOCO_TRY(dec_check(e, fn, B, T_enc, S, workspace, (size_t)-1, p));  // the size is checked against the alignment's own plan below
    AlignPlan a;
    make_align_plan(e->dec.layers, B, T_enc, S, a);
    if (workspace_bytes < a.total) return fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, a.total);
    if (!enc_out || !decoder_input_ids || !token_counts || !start_frames || !end_frames) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    std::vector<unsigned> heads(a.dec.L, 0u);
    DecAttnSink sink;
    if (!layer_heads) {  // every pair
        for (auto& h : heads) h = (1u << kHeads) - 1;
        sink.pairs = a.dec.L * kHeads;
    } else {
        if (pairs < 1) return fail(LOCO_E_INVALID, "%s: an alignment head list needs at least one (layer, head) pair", fn);
        for (int i = 0; i < pairs; ++i) {
            const int l = layer_heads[2 * i], h = layer_heads[2 * i + 1];
            if (l < 0 || l >= a.dec.L || h < 0 || h >= kHeads)
                return fail(LOCO_E_INVALID, "%s: alignment head %d = (layer %d, head %d) is outside %d layers x %d heads", fn, i, l, h, a.dec.L, kHeads);
            if (heads[l] >> h & 1u) return fail(LOCO_E_INVALID, "%s: alignment head (layer %d, head %d) is named twice", fn, l, h);
            heads[l] |= 1u << h;
        }
        sink.pairs = pairs;
    }
    sink.first_layer = -1;
    for (int l = 0; l < a.dec.L; ++l)
        if (heads[l]) {
            if (sink.first_layer < 0) sink.first_layer = l;
            sink.last_layer = l;
        }
    char* ws = static_cast<char*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    sink.heads = heads.data();
    sink.scratch = reinterpret_cast<float*>(ws + a.off_probs);
    sink.mean = attention ? attention : reinterpret_cast<float*>(ws + a.off_mean);
    LOCO_TRY(dec_forward_walk(e, a.dec, ws, enc_out, enc_frames, decoder_input_ids, nullptr, nullptr, sink, s));
    HIP_TRY(launch_dtw_align(sink.mean, T_enc, token_counts, reinterpret_cast<const int32_t*>(ws + a.dec.off_frames), B, S, T_enc, start_frames,
                             end_frames, reinterpret_cast<unsigned char*>(ws + a.off_back), s));
    return LOCO_OK;
}

int loco_decoder_begin(loco_encoder* e, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc, int32_t S_max,
                       void* workspace, size_t workspace_bytes, void* stream) {
    DecPlan p;
    LOCO_TRY(dec_check(e, "loco_decoder_begin", B, T_enc, S_max, workspace, workspace_bytes, p));
    if (B > kSkinnyMaxM) return fail(LOCO_E_INVALID, "loco_decoder_begin: %d clips exceed the decode step's limit of %d rows", B, kSkinnyMaxM);
    if (!enc_out) return fail(LOCO_E_INVALID, "loco_decoder_begin: null encoder output");
    return dec_begin(e, p, static_cast<char*>(workspace), enc_out, enc_frames, (hipStream_t)stream);
}

int loco_decoder_step(loco_encoder* e, int32_t B, int32_t T_enc, int32_t S_max, int32_t t, float* logits, void* workspace,
                      size_t workspace_bytes, void* stream) {
    DecPlan p;
    LOCO_TRY(dec_check(e, "loco_decoder_step", B, T_enc, S_max, workspace, workspace_bytes, p));
    if (B > kSkinnyMaxM) return fail(LOCO_E_INVALID, "loco_decoder_step: %d clips exceed the decode step's limit of %d rows", B, kSkinnyMaxM);
    if (t < 0 || t + 1 >= S_max) return fail(LOCO_E_INVALID, "loco_decoder_step: step %d writes token %d of a buffer of %d", t, t + 1, S_max);
    return dec_step(e, p, static_cast<char*>(workspace), t, logits, (hipStream_t)stream);
}

int loco_decoder_read_tokens(const loco_encoder* e, int32_t B, int32_t T_enc, int32_t S_max, int32_t* tokens, int32_t* lengths, const void* workspace,
                             size_t workspace_bytes, void* stream) {
    DecPlan p;
    LOCO_TRY(dec_check(e, "loco_decoder_read_tokens", B, T_enc, S_max, workspace, workspace_bytes, p));
    const char* ws = static_cast<const char*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    if (tokens) HIP_TRY(hipMemcpyAsync(tokens, ws + p.off_tokens, (size_t)B * S_max * sizeof(int32_t), hipMemcpyDefault, s));
    if (lengths) HIP_TRY(hipMemcpyAsync(lengths, ws + p.off_lengths, (size_t)B * sizeof(int32_t), hipMemcpyDefault, s));
    return LOCO_OK;
}

// How often generate looks at the device's "rows still open" word.  A look is a 16-byte copy to pinned memory plus a stream
// synchronisation (~20 us of an idle queue); a step is 69 dependent launches (>= 100 us).  Every 8 steps keeps the queue fed for 8 steps
// at a time and wastes at most 7 steps of pad tokens after the last row has finished.
constexpr int kDecPollSteps = 8;

int loco_decoder_generate(loco_encoder* e, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc, int32_t max_length,
                          int32_t* tokens_out, int32_t* lengths_out, int32_t* out_length, float* step_logits, void* workspace,
                          size_t workspace_bytes, void* stream) {
    DecPlan p;
    LOCO_TRY(dec_check(e, "loco_decoder_generate", B, T_enc, max_length, workspace, workspace_bytes, p));
    if (B > kSkinnyMaxM) return fail(LOCO_E_INVALID, "loco_decoder_generate: %d clips exceed the decode step's limit of %d rows", B, kSkinnyMaxM);
    if (!enc_out || !tokens_out) return fail(LOCO_E_INVALID, "loco_decoder_generate: null argument");
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    LOCO_TRY(dec_begin(e, p, ws, enc_out, enc_frames, s));
    int32_t* host = e->dec.host_state;
    for (int t = 0; t + 1 < max_length; ++t) {
        LOCO_TRY(dec_step(e, p, ws, t, step_logits ? step_logits + (size_t)t * B * e->dec.vocab : nullptr, s));
        if ((t + 1) % kDecPollSteps == 0 && t + 2 < max_length) {
            HIP_TRY(hipMemcpyAsync(host, ws + p.off_state, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (host[0] == 0) break;
        }
    }
    std::vector<int32_t> lens(B);
    HIP_TRY(hipMemcpyAsync(tokens_out, ws + p.off_tokens, (size_t)B * max_length * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(lens.data(), ws + p.off_lengths, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int longest = 1;
    for (int b = 0; b < B; ++b) longest = lens[b] > longest ? lens[b] : longest;
    // HF stops after the step in which the last open row emits <eos>: the sequences are as long as the longest row; rows that finished
    // earlier hold <pad> from there on (steps enqueued beyond that point only wrote <pad>)
    if (lengths_out) memcpy(lengths_out, lens.data(), (size_t)B * sizeof(int32_t));
    if (out_length) *out_length = longest;
    return LOCO_OK;
}

// ---- decoder slot pool ---------------------------------------------------------------------------------------------------------
namespace {

// Workspace of one pool (caller-owned): the slot state first (the poll block -- [0] slots open, [4, 4 + slots) status, then lengths --
// is one contiguous run), the caches, then the step's row buffers and the attention scratch.
struct PoolPlan {
    int slots, T, S, L;
    size_t off_poll, off_pos, off_cap, off_frames, off_counts, off_tokens, off_nonpad, off_cross, off_self, off_x0, off_x1, off_tmp, off_q, off_ctx,
        off_ffn, off_logits, off_attn, off_sample, total;
};

void make_pool_plan(int layers, int slots, int T, int S, PoolPlan& p) {
    p.slots = slots, p.T = T, p.S = S, p.L = layers;
    const size_t f = sizeof(float), i = sizeof(int32_t);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o += align_up(bytes);
        return at;
    };
    p.off_poll = take((size_t)(4 + 2 * slots) * i);
    p.off_pos = take(slots * i);
    p.off_cap = take(slots * i);
    p.off_frames = take(slots * i);
    p.off_counts = take((size_t)3 * slots * i);  // self key counts, cross key counts, cache rows of the step
    p.off_tokens = take((size_t)slots * S * i);
    p.off_nonpad = take((size_t)2 * slots * i);  // the token each slot consumes next and its running non-pad count
    p.off_cross = take((size_t)slots * T * p.L * 2 * kHidden * f);  // [slots][T_cap][layers][k | v]
    p.off_self = take((size_t)p.L * slots * S * 2 * kHidden * f);   // [layers][slots][S_max][k | v]
    p.off_x0 = take((size_t)slots * kHidden * f);
    p.off_x1 = take((size_t)slots * kHidden * f);
    p.off_tmp = take((size_t)slots * kHidden * f);
    p.off_q = take((size_t)slots * kHidden * f);
    p.off_ctx = take((size_t)slots * kHidden * f);
    p.off_ffn = take((size_t)slots * kFfn * f);
    p.off_logits = take((size_t)slots * 128 * f);
    p.off_attn = take(dec_pool_attention_scratch_bytes(slots, T > S ? T : S));
    p.off_sample = take((size_t)2 * slots * sizeof(uint32_t));  // (utterance, hypothesis) of every slot: after every region a greedy pool has
    p.total = o;
}

PoolState pool_state(const PoolPlan& p, char* ws) {
    auto I = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    PoolState st{};
    st.poll = I(p.off_poll), st.status = st.poll + 4, st.lengths = st.status + p.slots;
    st.pos = I(p.off_pos), st.cap = I(p.off_cap), st.frames = I(p.off_frames);
    st.self_count = I(p.off_counts), st.cross_count = st.self_count + p.slots, st.kv_row = st.cross_count + p.slots;
    st.tokens = I(p.off_tokens), st.cur = I(p.off_nonpad), st.cnt = st.cur + p.slots;
    st.slots = p.slots, st.S_max = p.S, st.T_cap = p.T;
    return st;
}

int pool_check(const loco_encoder* e, const char* fn, int slots, int T, int S, const void* ws, size_t bytes, PoolPlan& p) {
    LOCO_TRY(dec_handle_check(e, fn));
    if (slots <= 0 || T <= 0) return fail(LOCO_E_INVALID, "%s: slots and T_cap must be positive", fn);
    if (slots > kSkinnyMaxM) return fail(LOCO_E_INVALID, "%s: %d slots exceed the decode step's limit of %d rows", fn, slots, kSkinnyMaxM);
    if (S < 2 || S > kDecMaxPositions)
        return fail(LOCO_E_INVALID, "%s: S_max = %d is outside 2 .. max_text_positions = %d", fn, S, kDecMaxPositions);
    if (!ws) return fail(LOCO_E_INVALID, "%s: null workspace", fn);
    make_pool_plan(e->dec.layers, slots, T, S, p);
    if (bytes < p.total) return fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, bytes, p.total);
    return LOCO_OK;
}

// bit r: slot r of the pool in `ws` draws (0: the handle knows no such pool)
unsigned long long pool_sampled_slots(const loco_encoder* e, const void* ws) {
    for (const auto& it : e->pool_sampled)
        if (it.first == ws) return it.second;
    return 0;
}

// mask 0 forgets the pool
void pool_sampled_set(loco_encoder* e, const void* ws, unsigned long long mask) {
    auto& v = e->pool_sampled;
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i].first == ws) {
            if (mask) v[i].second = mask;
            else v.erase(v.begin() + i);
            return;
        }
    if (mask) v.emplace_back(ws, mask);
}

// the config of the beam pool in `ws` (null: the handle knows no such pool); loco_decoder_pool_init forgets it
const loco_beam_config* pool_beam_config(const loco_encoder* e, const void* ws) {
    for (const auto& it : e->pool_beam)
        if (it.first == ws) return &it.second;
    return nullptr;
}

void pool_beam_forget(loco_encoder* e, const void* ws) {
    auto& v = e->pool_beam;
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i].first == ws) {
            v.erase(v.begin() + i);
            break;
        }
    auto& f = e->pool_fusion;
    for (size_t i = 0; i < f.size(); ++i)
        if (f[i].ws == ws) {
            f.erase(f.begin() + i);
            break;
        }
}

// the n-gram model attached to the beam pool in `ws` (null: none)
const loco_encoder::PoolFusion* pool_fusion(const loco_encoder* e, const void* ws) {
    for (const auto& it : e->pool_fusion)
        if (it.ws == ws) return &it;
    return nullptr;
}

// the greedy and sampling entry points on a beam pool
int pool_not_beam(const loco_encoder* e, const char* fn, const void* ws) {
    if (pool_beam_config(e, ws))
        return fail(LOCO_E_STATE, "%s: the pool holds beam groups (loco_decoder_pool_admit_beams); step it with loco_decoder_pool_step_beam", fn);
    return LOCO_OK;
}

// what loco_decoder_pool_admit and loco_decoder_pool_admit_samples ask of clip i of n
int pool_admit_check(const char* fn, int T_cap, int S_max, int n, int i, int rows, int cap, int64_t clip_stride) {
    if (rows < 1 || rows > T_cap)
        return fail(LOCO_E_INVALID, "%s: clip %d has %d encoder rows, the pool holds 1 .. T_cap = %d per slot", fn, i, rows, T_cap);
    if (n > 1 && clip_stride < (int64_t)rows * kHidden)  // clips would overlap in enc_out
        return fail(LOCO_E_INVALID, "%s: clip stride %lld is shorter than clip %d's %d rows", fn, (long long)clip_stride, i, rows);
    if (cap < 2 || cap > S_max) return fail(LOCO_E_INVALID, "%s: clip %d has cap %d, outside 2 .. S_max = %d", fn, i, cap, S_max);
    return LOCO_OK;
}

// The step up to its logits, for loco_decoder_pool_step and loco_decoder_pool_step_sample: the embedding of every open slot's token,
// the layers, the lm_head.  The caller's select kernel follows.
int pool_step_walk(loco_encoder* e, const PoolPlan& p, char* ws, const PoolState& st, int max_pos, int max_frames, float* logits, hipStream_t s) {
    const DecoderW& d = e->dec;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    float *x0 = F(p.off_x0), *x1 = F(p.off_x1), *tmp = F(p.off_tmp), *q = F(p.off_q), *ctx = F(p.off_ctx), *ffn = F(p.off_ffn), *scr = F(p.off_attn);
    const long ld_cross = (long)p.L * 2 * kHidden, ld_self = 2 * kHidden;
    const int B = p.slots;
    HIP_TRY(launch_pool_embed(st, d.embed, d.vocab, d.pos_tab, d.pos_rows, x0, max_pos, max_frames, s));
    for (int l = 0; l < p.L; ++l) {
        const DecLayerW& lw = d.L[l];
        float* cache = F(p.off_self) + (size_t)l * B * p.S * ld_self;
        // q -> row buffer, k|v -> row pos[r] of slot r's cache
        HIP_TRY(launch_skinny_gemm_rows(x0, kHidden, lw.wqkv, kHidden, lw.bqkv, q, kHidden, cache, (long)p.S * ld_self, st.kv_row, ld_self, kHidden, B,
                                        kQkv, kHidden, s));
        HIP_TRY(launch_dec_pool_attention(q, cache, ld_self, (long)p.S * ld_self, cache + kHidden, st.self_count, ctx, B, max_pos + 1, scr, s));
        LOCO_TRY(run_skinny(s, ctx, lw.self_out, x0, tmp, B, kHidden, kHidden, kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.self_ln.w, lw.self_ln.b, x1, B, kHidden));
        LOCO_TRY(run_skinny(s, x1, WB{lw.wcq, lw.bcq}, nullptr, q, B, kHidden, kHidden, kEpiNone));
        const float* ck = F(p.off_cross) + (size_t)l * 2 * kHidden;
        HIP_TRY(launch_dec_pool_attention(q, ck, ld_cross, (long)p.T * ld_cross, ck + kHidden, st.cross_count, ctx, B, max_frames, scr, s));
        LOCO_TRY(run_skinny(s, ctx, lw.cross_out, x1, tmp, B, kHidden, kHidden, kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.cross_ln.w, lw.cross_ln.b, x0, B, kHidden));
        LOCO_TRY(run_skinny(s, x0, lw.ffn_in, nullptr, ffn, B, kFfn, kHidden, kEpiGelu));
        LOCO_TRY(run_skinny(s, ffn, lw.ffn_out, x0, tmp, B, kHidden, kFfn, kEpiResidual));
        LOCO_TRY(run_ln(e, s, tmp, lw.final_ln.w, lw.final_ln.b, x0, B, kHidden));
    }
    LOCO_TRY(run_skinny(s, x0, WB{d.lm_head, nullptr}, nullptr, logits, B, d.vocab, kHidden, kEpiNone));
    return LOCO_OK;
}

// the bounds a step's launches are sized by (loco_decoder_pool_step, loco_decoder_pool_step_sample)
int pool_step_bounds_check(const char* fn, int T_cap, int S_max, int max_pos, int max_frames) {
    if (max_pos < 0 || max_pos + 1 >= S_max) return fail(LOCO_E_INVALID, "%s: position bound %d writes token %d of a buffer of %d", fn, max_pos, max_pos + 1, S_max);
    if (max_frames < 1 || max_frames > T_cap) return fail(LOCO_E_INVALID, "%s: frame bound %d is outside 1 .. T_cap = %d", fn, max_frames, T_cap);
    return LOCO_OK;
}

int sample_config_check(const loco_sample_config* c, const char* fn, SampleRule& rule) {
    if (!c) return fail(LOCO_E_INVALID, "%s: null loco_sample_config", fn);
    if (c->struct_size != sizeof(loco_sample_config))
        return fail(LOCO_E_INVALID, "%s: loco_sample_config.struct_size = %u, this library's is %zu", fn, c->struct_size, sizeof(loco_sample_config));
    if (!(c->temperature > 0.f) || !std::isfinite(c->temperature))
        return fail(LOCO_E_INVALID, "%s: loco_sample_config.temperature = %g must be finite and > 0", fn, (double)c->temperature);
    if (c->top_k < 0) return fail(LOCO_E_INVALID, "%s: loco_sample_config.top_k = %d must be >= 0 (0 = off)", fn, c->top_k);
    if (!(c->top_p > 0.f && c->top_p <= 1.f))
        return fail(LOCO_E_INVALID, "%s: loco_sample_config.top_p = %g is outside (0, 1] (1 = off)", fn, (double)c->top_p);
    rule = SampleRule{c->temperature, c->top_k, c->top_p, (uint32_t)(c->seed & 0xffffffffu), (uint32_t)(c->seed >> 32)};
    return LOCO_OK;
}

}  // namespace

size_t loco_decoder_pool_workspace_bytes(const loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max) {
    if (!e || slots <= 0 || slots > kSkinnyMaxM || T_cap <= 0 || S_max < 2 || S_max > kDecMaxPositions) return 0;
    if (!loco_has_decoder(e)) return 0;
    PoolPlan p;
    make_pool_plan(decoder_layers_loaded(e, nullptr), slots, T_cap, S_max, p);
    return p.total;
}

int loco_decoder_pool_init(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, void* workspace, size_t workspace_bytes, void* stream) {
    PoolPlan p;
    LOCO_TRY(pool_check(e, "loco_decoder_pool_init", slots, T_cap, S_max, workspace, workspace_bytes, p));
    HIP_TRY(launch_pool_init(pool_state(p, static_cast<char*>(workspace)), (hipStream_t)stream));
    pool_sampled_set(e, workspace, 0);
    pool_beam_forget(e, workspace);
    return LOCO_OK;
}

int loco_decoder_pool_admit(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t n, const int32_t* slot_ids, const float* enc_out,
                            int64_t clip_stride, const int32_t* enc_rows, const int32_t* enc_frames, const int32_t* caps, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const char* fn = "loco_decoder_pool_admit";
    PoolPlan p;
    LOCO_TRY(pool_check(e, fn, slots, T_cap, S_max, workspace, workspace_bytes, p));
    LOCO_TRY(pool_not_beam(e, fn, workspace));
    if (n <= 0 || n > slots) return fail(LOCO_E_INVALID, "%s: %d clips for a pool of %d slots", fn, n, slots);
    if (!slot_ids || !enc_out || !enc_rows || !caps) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (clip_stride < 0 || (clip_stride & 3) || (reinterpret_cast<uintptr_t>(enc_out) & 15))
        return fail(LOCO_E_INVALID, "%s: enc_out and the clip stride must be 16-byte aligned", fn);
    PoolAdmit a{};
    a.n = n;
    unsigned long long seen = 0;
    for (int i = 0; i < n; ++i) {
        if (slot_ids[i] < 0 || slot_ids[i] >= slots) return fail(LOCO_E_INVALID, "%s: slot %d of a pool of %d slots", fn, slot_ids[i], slots);
        if (seen >> slot_ids[i] & 1) return fail(LOCO_E_INVALID, "%s: slot %d is named twice", fn, slot_ids[i]);
        seen |= 1ull << slot_ids[i];
        LOCO_TRY(pool_admit_check(fn, T_cap, S_max, n, i, enc_rows[i], caps[i], clip_stride));
        a.slot[i] = slot_ids[i], a.cap[i] = caps[i], a.rows[i] = enc_rows[i];
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const PoolState st = pool_state(p, ws);
    // a slot that is open may not be overwritten: the slots' status is read back (the one place the pool waits for the stream; the
    // caller admits after a poll, when the stream is idle anyway)
    std::vector<int32_t> status(slots);
    HIP_TRY(hipMemcpyAsync(status.data(), st.status, (size_t)slots * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i)
        if (status[slot_ids[i]] == kPoolOpen) return fail(LOCO_E_STATE, "%s: slot %d is open (its utterance has not finished)", fn, slot_ids[i]);
    // cross-attention k|v of every layer, one exact-fp32 product per clip into the slot's own region: the rows of a clip are the same
    // bits whichever clips are admitted beside it
    const int N = p.L * 2 * kHidden;
    for (int i = 0; i < n; ++i)
        LOCO_TRY(run_gemm(e, s, enc_out + (size_t)i * clip_stride, kHidden, e->dec.wckv, kHidden, e->dec.bckv, nullptr, 0,
                         reinterpret_cast<float*>(ws + p.off_cross) + (size_t)slot_ids[i] * T_cap * N, N, enc_rows[i], N, kHidden, kEpiNone));
    HIP_TRY(launch_pool_admit(st, a, enc_frames, kDecStartToken, s));
    pool_sampled_set(e, workspace, pool_sampled_slots(e, workspace) & ~seen);  // these slots are greedy from here on
    return LOCO_OK;
}

int loco_decoder_pool_step(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t max_pos, int32_t max_frames, float* step_logits,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "loco_decoder_pool_step";
    PoolPlan p;
    LOCO_TRY(pool_check(e, fn, slots, T_cap, S_max, workspace, workspace_bytes, p));
    LOCO_TRY(pool_not_beam(e, fn, workspace));
    LOCO_TRY(pool_step_bounds_check(fn, T_cap, S_max, max_pos, max_frames));
    if (pool_sampled_slots(e, workspace))
        return fail(LOCO_E_STATE, "%s: the pool holds slots admitted to sample (mask 0x%llx); step it with loco_decoder_pool_step_sample", fn,
                    pool_sampled_slots(e, workspace));
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const PoolState st = pool_state(p, ws);
    float* logits = step_logits ? step_logits : reinterpret_cast<float*>(ws + p.off_logits);
    LOCO_TRY(pool_step_walk(e, p, ws, st, max_pos, max_frames, logits, s));
    HIP_TRY(launch_pool_select(st, logits, e->dec.vocab, kDecEosToken, s));
    return LOCO_OK;
}

int loco_decoder_pool_admit_samples(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t n, int32_t copies, const int32_t* slot_ids,
                                    const float* enc_out, int64_t clip_stride, const int32_t* enc_rows, const int32_t* enc_frames, const int32_t* caps,
                                    const uint32_t* utterances, const uint32_t* hypotheses, const int32_t* greedy, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const char* fn = "loco_decoder_pool_admit_samples";
    PoolPlan p;
    LOCO_TRY(pool_check(e, fn, slots, T_cap, S_max, workspace, workspace_bytes, p));
    LOCO_TRY(pool_not_beam(e, fn, workspace));
    if (n <= 0 || copies <= 0 || (int64_t)n * copies > slots)
        return fail(LOCO_E_INVALID, "%s: %d clips x %d copies for a pool of %d slots", fn, n, copies, slots);
    if (!slot_ids || !enc_out || !enc_rows || !caps || !utterances || !hypotheses) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (clip_stride < 0 || (clip_stride & 3) || (reinterpret_cast<uintptr_t>(enc_out) & 15))
        return fail(LOCO_E_INVALID, "%s: enc_out and the clip stride must be 16-byte aligned", fn);
    PoolAdmitSamples a{};
    a.n = n * copies, a.copies = copies;
    unsigned long long seen = 0, draws = 0;
    for (int i = 0; i < n; ++i) {
        LOCO_TRY(pool_admit_check(fn, T_cap, S_max, n, i, enc_rows[i], caps[i], clip_stride));
        for (int c = 0; c < copies; ++c) {
            const int k = i * copies + c, r = slot_ids[k];
            if (r < 0 || r >= slots) return fail(LOCO_E_INVALID, "%s: slot %d of a pool of %d slots", fn, r, slots);
            if (seen >> r & 1) return fail(LOCO_E_INVALID, "%s: slot %d is named twice", fn, r);
            seen |= 1ull << r;
            if (!(greedy && greedy[k])) draws |= 1ull << r;
            a.slot[k] = r, a.cap[k] = caps[i], a.rows[k] = enc_rows[i], a.utterance[k] = utterances[i], a.hypothesis[k] = hypotheses[k];
        }
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const PoolState st = pool_state(p, ws);
    // as loco_decoder_pool_admit: an open slot may not be overwritten; one read-back, one wait for the stream, for the whole call
    std::vector<int32_t> status(slots);
    HIP_TRY(hipMemcpyAsync(status.data(), st.status, (size_t)slots * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < a.n; ++k)
        if (status[a.slot[k]] == kPoolOpen) return fail(LOCO_E_STATE, "%s: slot %d is open (its utterance has not finished)", fn, a.slot[k]);
    // a clip's cross k|v: loco_decoder_pool_admit's product into the first slot, then copies of those bytes into the siblings' regions
    const int N = p.L * 2 * kHidden;
    float* cross = reinterpret_cast<float*>(ws + p.off_cross);
    for (int i = 0; i < n; ++i) {
        float* first = cross + (size_t)a.slot[i * copies] * T_cap * N;
        LOCO_TRY(run_gemm(e, s, enc_out + (size_t)i * clip_stride, kHidden, e->dec.wckv, kHidden, e->dec.bckv, nullptr, 0, first, N, enc_rows[i], N, kHidden,
                         kEpiNone));
        for (int c = 1; c < copies; ++c)
            HIP_TRY(hipMemcpyAsync(cross + (size_t)a.slot[i * copies + c] * T_cap * N, first, (size_t)enc_rows[i] * N * sizeof(float),
                                   hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(launch_pool_admit_samples(st, a, enc_frames, kDecStartToken, reinterpret_cast<uint32_t*>(ws + p.off_sample), s));
    pool_sampled_set(e, workspace, (pool_sampled_slots(e, workspace) & ~seen) | draws);
    return LOCO_OK;
}

int loco_decoder_pool_step_sample(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t max_pos, int32_t max_frames,
                                  const loco_sample_config* config, float* step_logits, int32_t* step_tokens, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    const char* fn = "loco_decoder_pool_step_sample";
    PoolPlan p;
    LOCO_TRY(pool_check(e, fn, slots, T_cap, S_max, workspace, workspace_bytes, p));
    LOCO_TRY(pool_not_beam(e, fn, workspace));
    LOCO_TRY(pool_step_bounds_check(fn, T_cap, S_max, max_pos, max_frames));
    SampleRule rule;
    LOCO_TRY(sample_config_check(config, fn, rule));
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const PoolState st = pool_state(p, ws);
    float* logits = step_logits ? step_logits : reinterpret_cast<float*>(ws + p.off_logits);
    LOCO_TRY(pool_step_walk(e, p, ws, st, max_pos, max_frames, logits, s));
    HIP_TRY(launch_pool_sample_select(st, reinterpret_cast<const uint32_t*>(ws + p.off_sample), pool_sampled_slots(e, workspace), rule, logits,
                                      e->dec.vocab, kDecEosToken, step_tokens, -100, s));  // -100: the ignore_index loco_decoder_score's callers pass
    return LOCO_OK;
}

int loco_op_sample_tokens(const float* logits, int64_t ld, int32_t M, int32_t V, const loco_sample_config* config, const uint32_t* counters,
                          const int32_t* greedy, int32_t* tokens, int32_t* keep, float* uniform, void* stream) {
    const char* fn = "loco_op_sample_tokens";
    if (!logits || !counters || !tokens) return fail(LOCO_E_INVALID, "%s: null logits, counters or tokens", fn);
    if (M < 1 || V < 1) return fail(LOCO_E_INVALID, "%s: M = %d and V = %d must both be >= 1", fn, M, V);
    if (ld < V) return fail(LOCO_E_INVALID, "%s: row stride ld = %lld < V = %d", fn, (long long)ld, V);
    SampleRule rule;
    LOCO_TRY(sample_config_check(config, fn, rule));
    HIP_TRY(launch_sample_tokens(logits, (long)ld, M, V, rule, counters, greedy, tokens, keep, uniform, (hipStream_t)stream));
    return LOCO_OK;
}

// ---- beam search in the slot pool ------------------------------------------------------------------------------------------------
namespace {

// the beam regions of a pool's workspace, after every region of the greedy (and sampling) pool
struct BeamPlan {
    PoolPlan pool;
    int K, groups;
    size_t off_shadow, off_fin_tok, off_fin_tlp, off_fin_score, off_fin_sum, off_fin_len, off_run, off_alive, off_tlp, off_parent, off_count, off_den,
        off_unsat, off_fin_n, off_tok_shadow, off_tlp_shadow, off_lp, total, off_bonus, total_fused;
};

void make_beam_plan(int layers, int slots, int T, int S, int K, BeamPlan& b) {
    make_pool_plan(layers, slots, T, S, b.pool);
    b.K = K, b.groups = slots / K;
    const size_t f = sizeof(float), i = sizeof(int32_t), d = sizeof(double);
    size_t o = b.pool.total;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o += align_up(bytes);
        return at;
    };
    b.off_shadow = take((size_t)b.pool.L * slots * S * 2 * kHidden * f);  // the self cache's shape
    b.off_fin_tok = take((size_t)slots * S * i);
    b.off_fin_tlp = take((size_t)slots * S * f);
    b.off_fin_score = take(slots * d);
    b.off_fin_sum = take(slots * d);
    b.off_fin_len = take(slots * i);
    b.off_run = take(slots * d);
    b.off_alive = take(slots * i);
    b.off_tlp = take((size_t)slots * S * f);
    b.off_parent = take(slots * i);
    b.off_count = take(slots * i);
    b.off_den = take((size_t)kDecMaxPositions * d);
    b.off_unsat = take(slots * i);
    b.off_fin_n = take(slots * i);
    b.off_tok_shadow = take((size_t)slots * S * i);
    b.off_tlp_shadow = take((size_t)slots * S * f);
    b.off_lp = take((size_t)slots * 128 * f);  // the logits region's shape
    b.total = o;
    b.off_bonus = take((size_t)slots * 128 * d);  // a pool with an n-gram model attached: the candidates' bonus, after everything else
    b.total_fused = o;
}

BeamState beam_state(const BeamPlan& b, char* ws) {
    auto I = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    auto D = [&](size_t off) { return reinterpret_cast<double*>(ws + off); };
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    BeamState s{};
    s.run = D(b.off_run), s.fin_score = D(b.off_fin_score), s.fin_sum = D(b.off_fin_sum), s.den = D(b.off_den);
    s.tlp = F(b.off_tlp), s.fin_tlp = F(b.off_fin_tlp);
    s.alive = I(b.off_alive), s.parent = I(b.off_parent), s.count = I(b.off_count), s.unsat = I(b.off_unsat), s.fin_n = I(b.off_fin_n);
    s.fin_len = I(b.off_fin_len), s.fin_tok = I(b.off_fin_tok);
    s.groups = b.groups, s.den_n = kDecMaxPositions;
    return s;
}

// V <= 0: the vocabulary is not checked
int beam_config_check(const loco_beam_config* c, const char* fn, int V, BeamRule& rule) {
    if (!c) return fail(LOCO_E_INVALID, "%s: null loco_beam_config", fn);
    if (c->struct_size != sizeof(loco_beam_config))
        return fail(LOCO_E_INVALID, "%s: loco_beam_config.struct_size = %u, this library's is %zu", fn, c->struct_size, sizeof(loco_beam_config));
    if (c->num_beams < 1 || c->num_beams > kBeamMax)
        return fail(LOCO_E_INVALID, "%s: loco_beam_config.num_beams = %d is outside 1 .. %d", fn, c->num_beams, kBeamMax);
    if (V > 0 && 2 * c->num_beams > V)
        return fail(LOCO_E_INVALID, "%s: loco_beam_config.num_beams = %d needs 2 * num_beams <= V = %d candidates", fn, c->num_beams, V);
    if (!std::isfinite(c->length_penalty))
        return fail(LOCO_E_INVALID, "%s: loco_beam_config.length_penalty = %g must be finite", fn, c->length_penalty);
    if (c->early_stopping < 0 || c->early_stopping > 2)
        return fail(LOCO_E_INVALID, "%s: loco_beam_config.early_stopping = %d is not 0 (false), 1 (true) or 2 (never)", fn, c->early_stopping);
    rule = BeamRule{c->num_beams, c->early_stopping, c->length_penalty > 0.0};
    return LOCO_OK;
}

int beam_pool_check(const loco_encoder* e, const char* fn, int slots, int T, int S, int K, const void* ws, size_t bytes, BeamPlan& b) {
    PoolPlan p;
    LOCO_TRY(pool_check(e, fn, slots, T, S, ws, bytes, p));
    if (K > slots) return fail(LOCO_E_INVALID, "%s: num_beams = %d exceeds the pool's %d slots", fn, K, slots);
    make_beam_plan(e->dec.layers, slots, T, S, K, b);
    if (bytes < b.total) return fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes (loco_decoder_beam_workspace_bytes)", fn, bytes, b.total);
    return LOCO_OK;
}

void fill_den_table(double length_penalty, int n, double* den) {
    for (int i = 0; i < n; ++i) den[i] = i == 0 ? 1.0 : std::pow((double)i, length_penalty);
}

}  // namespace

int loco_beam_den_table(double length_penalty, int32_t n, double* den_host) {
    if (!den_host || n < 1 || !std::isfinite(length_penalty)) return fail(LOCO_E_INVALID, "loco_beam_den_table: null table, n < 1 or a penalty that is not finite");
    fill_den_table(length_penalty, n, den_host);
    return LOCO_OK;
}

size_t loco_decoder_beam_workspace_bytes(const loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t num_beams) {
    if (!loco_decoder_pool_workspace_bytes(e, slots, T_cap, S_max) || num_beams < 1 || num_beams > kBeamMax || num_beams > slots) return 0;
    BeamPlan b;
    make_beam_plan(decoder_layers_loaded(e, nullptr), slots, T_cap, S_max, num_beams, b);
    return b.total;
}

size_t loco_decoder_beam_fusion_workspace_bytes(const loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t num_beams) {
    if (!loco_decoder_beam_workspace_bytes(e, slots, T_cap, S_max, num_beams)) return 0;
    BeamPlan b;
    make_beam_plan(decoder_layers_loaded(e, nullptr), slots, T_cap, S_max, num_beams, b);
    return b.total_fused;
}

int loco_decoder_pool_attach_ngram(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, const loco_ngram* lm, double weight,
                                   double token_bonus, void* workspace, size_t workspace_bytes) {
    const char* fn = "loco_decoder_pool_attach_ngram";
    LOCO_TRY(dec_handle_check(e, fn));
    BeamPlan bp;
    LOCO_TRY(beam_pool_check(e, fn, slots, T_cap, S_max, 1, workspace, workspace_bytes, bp));
    if (workspace_bytes < bp.total_fused)
        return fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes (loco_decoder_beam_fusion_workspace_bytes)", fn, workspace_bytes, bp.total_fused);
    if (!lm) return fail(LOCO_E_INVALID, "%s: null model", fn);
    if (lm->device != e->device)
        return fail(LOCO_E_INVALID, "%s: the model's table is on device %d, the decoder on device %d", fn, lm->device, e->device);
    if (lm->table.V != e->dec.vocab)
        return fail(LOCO_E_INVALID, "%s: the model's vocab = %d is not the decoder's %d", fn, lm->table.V, e->dec.vocab);
    if (!std::isfinite(weight)) return fail(LOCO_E_INVALID, "%s: weight = %g must be finite", fn, weight);
    if (!std::isfinite(token_bonus)) return fail(LOCO_E_INVALID, "%s: token_bonus = %g must be finite", fn, token_bonus);
    if (pool_beam_config(e, workspace))
        return fail(LOCO_E_STATE, "%s: the pool has admitted beam groups; attach after loco_decoder_pool_init and before the first admission", fn);
    if (pool_sampled_slots(e, workspace)) return fail(LOCO_E_STATE, "%s: the pool holds slots admitted to sample", fn);
    if (pool_fusion(e, workspace)) return fail(LOCO_E_STATE, "%s: the pool has a model attached; loco_decoder_pool_init comes first", fn);
    e->pool_fusion.push_back({workspace, lm, weight, token_bonus});
    return LOCO_OK;
}

int loco_decoder_pool_admit_beams(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, const loco_beam_config* config, int32_t n,
                                  const int32_t* group_ids, const float* enc_out, int64_t clip_stride, const int32_t* enc_rows,
                                  const int32_t* enc_frames, const int32_t* caps, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "loco_decoder_pool_admit_beams";
    LOCO_TRY(dec_handle_check(e, fn));
    BeamRule rule;
    LOCO_TRY(beam_config_check(config, fn, e->dec.vocab, rule));
    const int K = rule.K;
    BeamPlan bp;
    LOCO_TRY(beam_pool_check(e, fn, slots, T_cap, S_max, K, workspace, workspace_bytes, bp));
    if (e->dec.vocab > 128) return fail(LOCO_E_INVALID, "%s: a vocabulary of %d exceeds the pool's 128 columns", fn, e->dec.vocab);
    if (n <= 0 || n > bp.groups) return fail(LOCO_E_INVALID, "%s: %d clips for a pool of %d groups of %d slots", fn, n, bp.groups, K);
    if (!group_ids || !enc_out || !enc_rows || !caps) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (clip_stride < 0 || (clip_stride & 3) || (reinterpret_cast<uintptr_t>(enc_out) & 15))
        return fail(LOCO_E_INVALID, "%s: enc_out and the clip stride must be 16-byte aligned", fn);
    const loco_beam_config* known = pool_beam_config(e, workspace);
    if (known && (known->num_beams != config->num_beams || known->length_penalty != config->length_penalty || known->early_stopping != config->early_stopping))
        return fail(LOCO_E_STATE, "%s: the pool's groups were admitted with another loco_beam_config; loco_decoder_pool_init comes first", fn);
    if (pool_sampled_slots(e, workspace)) return fail(LOCO_E_STATE, "%s: the pool holds slots admitted to sample", fn);
    PoolAdmitSamples a{};
    a.n = n * K, a.copies = K;
    unsigned long long seen = 0;
    for (int i = 0; i < n; ++i) {
        LOCO_TRY(pool_admit_check(fn, T_cap, S_max, n, i, enc_rows[i], caps[i], clip_stride));
        const int g = group_ids[i];
        if (g < 0 || g >= bp.groups) return fail(LOCO_E_INVALID, "%s: group %d of a pool of %d groups", fn, g, bp.groups);
        if (seen >> g & 1) return fail(LOCO_E_INVALID, "%s: group %d is named twice", fn, g);
        seen |= 1ull << g;
        for (int k = 0; k < K; ++k) a.slot[i * K + k] = g * K + k, a.cap[i * K + k] = caps[i], a.rows[i * K + k] = enc_rows[i];
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const PoolState st = pool_state(bp.pool, ws);
    // as loco_decoder_pool_admit: one read-back of the slots' status, one wait for the stream
    std::vector<int32_t> status(slots);
    HIP_TRY(hipMemcpyAsync(status.data(), st.status, (size_t)slots * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!known) {
        // the pool becomes a beam pool: no slot may be open under another step's rules; the den table is written while the stream idles
        for (int r = 0; r < slots; ++r)
            if (status[r] == kPoolOpen) return fail(LOCO_E_STATE, "%s: slot %d is open in a pool that is not a beam pool yet", fn, r);
        std::vector<double> den(kDecMaxPositions);
        fill_den_table(config->length_penalty, kDecMaxPositions, den.data());
        HIP_TRY(hipMemcpyAsync(ws + bp.off_den, den.data(), den.size() * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (int k = 0; k < a.n; ++k)
        if (status[a.slot[k]] == kPoolOpen) return fail(LOCO_E_STATE, "%s: group %d is open (its utterance has not finished)", fn, a.slot[k] / K);
    // a clip's cross k|v: one product into the group's first slot, copies of those bytes into the other beams' regions
    const int N = bp.pool.L * 2 * kHidden;
    float* cross = reinterpret_cast<float*>(ws + bp.pool.off_cross);
    for (int i = 0; i < n; ++i) {
        float* first = cross + (size_t)a.slot[i * K] * T_cap * N;
        LOCO_TRY(run_gemm(e, s, enc_out + (size_t)i * clip_stride, kHidden, e->dec.wckv, kHidden, e->dec.bckv, nullptr, 0, first, N, enc_rows[i], N, kHidden,
                         kEpiNone));
        for (int k = 1; k < K; ++k)
            HIP_TRY(hipMemcpyAsync(cross + (size_t)a.slot[i * K + k] * T_cap * N, first, (size_t)enc_rows[i] * N * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(launch_pool_admit_beams(st, beam_state(bp, ws), a, enc_frames, kDecStartToken, s));
    if (!known) e->pool_beam.emplace_back(workspace, *config);
    return LOCO_OK;
}

int loco_decoder_pool_step_beam(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t max_pos, int32_t max_frames,
                                float* step_logits, float* step_logprobs, int32_t* step_parents, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const char* fn = "loco_decoder_pool_step_beam";
    LOCO_TRY(dec_handle_check(e, fn));
    const loco_beam_config* config = pool_beam_config(e, workspace);
    if (!config) return fail(LOCO_E_STATE, "%s: the pool holds no beam groups (loco_decoder_pool_admit_beams); step it with loco_decoder_pool_step", fn);
    BeamRule rule;
    LOCO_TRY(beam_config_check(config, fn, e->dec.vocab, rule));
    BeamPlan bp;
    LOCO_TRY(beam_pool_check(e, fn, slots, T_cap, S_max, rule.K, workspace, workspace_bytes, bp));
    LOCO_TRY(pool_step_bounds_check(fn, T_cap, S_max, max_pos, max_frames));
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const PoolState st = pool_state(bp.pool, ws);
    const BeamState bs = beam_state(bp, ws);
    const int V = e->dec.vocab;
    float* logits = step_logits ? step_logits : reinterpret_cast<float*>(ws + bp.pool.off_logits);
    float* lp = step_logprobs ? step_logprobs : reinterpret_cast<float*>(ws + bp.off_lp);
    const loco_encoder::PoolFusion* fusion = pool_fusion(e, workspace);
    if (fusion && workspace_bytes < bp.total_fused)
        return fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes (loco_decoder_beam_fusion_workspace_bytes)", fn, workspace_bytes, bp.total_fused);
    LOCO_TRY(pool_step_walk(e, bp.pool, ws, st, max_pos, max_frames, logits, s));
    double* bonus = nullptr;
    if (fusion) {
        // weight * log P_lm(v | the slot's tokens) + token_bonus for every slot the embed kernel took as live (kv_row + 1 tokens)
        bonus = reinterpret_cast<double*>(ws + bp.off_bonus);
        HIP_TRY(launch_ngram_logprobs(fusion->lm->table, st.tokens, S_max, S_max, st.kv_row, 1, slots, true, fusion->weight, fusion->token_bonus, bonus, s));
    }
    HIP_TRY(launch_beam_select(st, bs, rule, logits, V, V, kDecEosToken, lp, s, bonus));
    if (step_parents) HIP_TRY(hipMemcpyAsync(step_parents, bs.parent, (size_t)slots * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    // rows 0 .. pos of the self cache, the token rows and their log-probabilities follow the parents
    HIP_TRY(launch_beam_reorder(ws + bp.pool.off_self, ws + bp.off_shadow, bp.pool.L, slots, S_max, 2 * kHidden, bs.parent, bs.count, st.status, rule.K,
                                max_pos + 1, s));
    HIP_TRY(launch_beam_reorder(st.tokens, ws + bp.off_tok_shadow, 1, slots, S_max, 1, bs.parent, bs.count, st.status, rule.K, max_pos + 1, s));
    HIP_TRY(launch_beam_reorder(bs.tlp, ws + bp.off_tlp_shadow, 1, slots, S_max, 1, bs.parent, bs.count, st.status, rule.K, max_pos + 1, s));
    return LOCO_OK;
}

int loco_decoder_pool_read_beams(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t group, int32_t* count, int32_t* tokens,
                                 int32_t* lengths, double* scores, double* sum_logprobs, float* token_logprobs, const void* workspace,
                                 size_t workspace_bytes, void* stream) {
    const char* fn = "loco_decoder_pool_read_beams";
    LOCO_TRY(dec_handle_check(e, fn));
    const loco_beam_config* config = pool_beam_config(e, workspace);
    if (!config) return fail(LOCO_E_STATE, "%s: the pool holds no beam groups (loco_decoder_pool_admit_beams)", fn);
    const int K = config->num_beams;
    BeamPlan bp;
    LOCO_TRY(beam_pool_check(e, fn, slots, T_cap, S_max, K, workspace, workspace_bytes, bp));
    if (group < 0 || group >= bp.groups) return fail(LOCO_E_INVALID, "%s: group %d of a pool of %d groups", fn, group, bp.groups);
    hipStream_t s = (hipStream_t)stream;
    const char* ws = static_cast<const char*>(workspace);
    const size_t r0 = (size_t)group * K;
    auto get = [&](void* dst, size_t off, size_t first, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, ws + off + first, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    HIP_TRY(get(count, bp.off_fin_n, (size_t)group * sizeof(int32_t), sizeof(int32_t)));
    HIP_TRY(get(tokens, bp.off_fin_tok, r0 * S_max * sizeof(int32_t), (size_t)K * S_max * sizeof(int32_t)));
    HIP_TRY(get(lengths, bp.off_fin_len, r0 * sizeof(int32_t), K * sizeof(int32_t)));
    HIP_TRY(get(scores, bp.off_fin_score, r0 * sizeof(double), K * sizeof(double)));
    HIP_TRY(get(sum_logprobs, bp.off_fin_sum, r0 * sizeof(double), K * sizeof(double)));
    HIP_TRY(get(token_logprobs, bp.off_fin_tlp, r0 * S_max * sizeof(float), (size_t)K * S_max * sizeof(float)));
    return LOCO_OK;
}

namespace {
int op_beam_select(const char* fn, const float* logits, int64_t ld, int32_t G, int32_t V, int32_t S_max, const loco_beam_config* config,
                   const double* den, int32_t* status, int32_t* pos, const int32_t* cap, int32_t* cur, int32_t* cnt, int32_t* lengths, int32_t* tokens,
                   float* token_logprobs, double* run, int32_t* alive, int32_t* unsat, int32_t* fin_count, double* fin_scores, double* fin_sums,
                   int32_t* fin_lengths, int32_t* fin_tokens, float* fin_logprobs, float* logprobs, int32_t* parents, int32_t* counts, int32_t* poll,
                   const double* bonus, void* stream) {
    BeamRule rule;
    LOCO_TRY(beam_config_check(config, fn, V, rule));
    if (!logits || !den || !status || !pos || !cap || !cur || !cnt || !lengths || !tokens || !token_logprobs || !run || !alive || !unsat || !fin_count ||
        !fin_scores || !fin_sums || !fin_lengths || !fin_tokens || !fin_logprobs || !logprobs || !parents || !counts)
        return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (G < 1 || (int64_t)G * rule.K > 65535) return fail(LOCO_E_INVALID, "%s: G = %d groups of %d slots", fn, G, rule.K);
    if (poll && G * rule.K > 64) return fail(LOCO_E_INVALID, "%s: poll counts at most 64 slots, G * num_beams = %d", fn, G * rule.K);
    if (V > (1 << 20)) return fail(LOCO_E_INVALID, "%s: V = %d exceeds 2^20", fn, V);
    if (ld < V) return fail(LOCO_E_INVALID, "%s: row stride ld = %lld < V = %d", fn, (long long)ld, V);
    if (S_max < 2 || S_max > kDecMaxPositions) return fail(LOCO_E_INVALID, "%s: S_max = %d is outside 2 .. %d", fn, S_max, kDecMaxPositions);
    PoolState p{};
    p.poll = poll, p.status = status, p.pos = pos, p.kv_row = pos, p.cap = const_cast<int32_t*>(cap), p.lengths = lengths, p.tokens = tokens;
    p.cur = cur, p.cnt = cnt;
    p.slots = G * rule.K, p.S_max = S_max, p.T_cap = 0;
    BeamState b{};
    b.run = run, b.fin_score = fin_scores, b.fin_sum = fin_sums, b.den = den, b.tlp = token_logprobs, b.fin_tlp = fin_logprobs;
    b.alive = alive, b.parent = parents, b.count = counts, b.unsat = unsat, b.fin_n = fin_count, b.fin_len = fin_lengths, b.fin_tok = fin_tokens;
    b.groups = G, b.den_n = S_max;
    HIP_TRY(launch_beam_select(p, b, rule, logits, (long)ld, V, kDecEosToken, logprobs, (hipStream_t)stream, bonus));
    return LOCO_OK;
}
}  // namespace

int loco_op_beam_select(const float* logits, int64_t ld, int32_t G, int32_t V, int32_t S_max, const loco_beam_config* config, const double* den,
                        int32_t* status, int32_t* pos, const int32_t* cap, int32_t* cur, int32_t* cnt, int32_t* lengths, int32_t* tokens,
                        float* token_logprobs, double* run, int32_t* alive, int32_t* unsat, int32_t* fin_count, double* fin_scores,
                        double* fin_sums, int32_t* fin_lengths, int32_t* fin_tokens, float* fin_logprobs, float* logprobs, int32_t* parents,
                        int32_t* counts, int32_t* poll, void* stream) {
    return op_beam_select("loco_op_beam_select", logits, ld, G, V, S_max, config, den, status, pos, cap, cur, cnt, lengths, tokens, token_logprobs, run,
                          alive, unsat, fin_count, fin_scores, fin_sums, fin_lengths, fin_tokens, fin_logprobs, logprobs, parents, counts, poll, nullptr,
                          stream);
}

int loco_op_beam_select_fused(const float* logits, int64_t ld, int32_t G, int32_t V, int32_t S_max, const loco_beam_config* config, const double* den,
                              int32_t* status, int32_t* pos, const int32_t* cap, int32_t* cur, int32_t* cnt, int32_t* lengths, int32_t* tokens,
                              float* token_logprobs, double* run, int32_t* alive, int32_t* unsat, int32_t* fin_count, double* fin_scores,
                              double* fin_sums, int32_t* fin_lengths, int32_t* fin_tokens, float* fin_logprobs, float* logprobs, int32_t* parents,
                              int32_t* counts, int32_t* poll, const double* bonus, void* stream) {
    return op_beam_select("loco_op_beam_select_fused", logits, ld, G, V, S_max, config, den, status, pos, cap, cur, cnt, lengths, tokens, token_logprobs,
                          run, alive, unsat, fin_count, fin_scores, fin_sums, fin_lengths, fin_tokens, fin_logprobs, logprobs, parents, counts, poll,
                          bonus, stream);
}

int loco_op_beam_reorder(void* buf, void* shadow, int32_t layers, int32_t slots, int32_t S_max, int64_t width, const int32_t* parents,
                         const int32_t* counts, const int32_t* status, int32_t num_beams, int32_t max_count, void* stream) {
    const char* fn = "loco_op_beam_reorder";
    if (!buf || !shadow || buf == shadow || !parents || !counts) return fail(LOCO_E_INVALID, "%s: null argument, or buf == shadow", fn);
    if (layers < 1 || layers > 65535 || slots < 1 || slots > 65535 || S_max < 1 || width < 1 || max_count < 0)
        return fail(LOCO_E_INVALID, "%s: layers = %d, slots = %d, S_max = %d, width = %lld, max_count = %d", fn, layers, slots, S_max, (long long)width, max_count);
    if (num_beams < 1 || num_beams > kBeamMax) return fail(LOCO_E_INVALID, "%s: num_beams = %d is outside 1 .. %d", fn, num_beams, kBeamMax);
    HIP_TRY(launch_beam_reorder(buf, shadow, layers, slots, S_max, (long)width, parents, counts, status, num_beams, max_count, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_decoder_pool_poll(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t* host_block, const void* workspace,
                           size_t workspace_bytes, void* stream) {
    PoolPlan p;
    LOCO_TRY(pool_check(e, "loco_decoder_pool_poll", slots, T_cap, S_max, workspace, workspace_bytes, p));
    if (!host_block) return fail(LOCO_E_INVALID, "loco_decoder_pool_poll: null host block");
    HIP_TRY(hipMemcpyAsync(host_block, static_cast<const char*>(workspace) + p.off_poll, (size_t)(4 + 2 * slots) * sizeof(int32_t),
                           hipMemcpyDeviceToHost, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_decoder_pool_read(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t slot, int32_t* tokens, const void* workspace,
                           size_t workspace_bytes, void* stream) {
    PoolPlan p;
    LOCO_TRY(pool_check(e, "loco_decoder_pool_read", slots, T_cap, S_max, workspace, workspace_bytes, p));
    if (slot < 0 || slot >= slots) return fail(LOCO_E_INVALID, "loco_decoder_pool_read: slot %d of a pool of %d slots", slot, slots);
    if (!tokens) return fail(LOCO_E_INVALID, "loco_decoder_pool_read: null token buffer");
    HIP_TRY(hipMemcpyAsync(tokens, static_cast<const char*>(workspace) + p.off_tokens + (size_t)slot * S_max * sizeof(int32_t),
                           (size_t)S_max * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_skinny_gemm(const float* A, int64_t lda, const float* Wt, int64_t ldw, const float* bias, const float* R, int64_t ldr, float* C,
                        int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epilogue, void* stream) {
    if (!A || !Wt || !C) return fail(LOCO_E_INVALID, "loco_op_skinny_gemm: null argument");
    if (M > kSkinnyMaxM) return fail(LOCO_E_INVALID, "loco_op_skinny_gemm: M = %d exceeds the limit of %d rows (use loco_op_gemm)", M, kSkinnyMaxM);
    if (epilogue < 0 || epilogue > 2) return fail(LOCO_E_INVALID, "loco_op_skinny_gemm: epilogue must be 0, 1 or 2");
    HIP_TRY(launch_skinny_gemm(A, lda, Wt, ldw, bias, R, ldr, C, ldc, nullptr, 0, N, M, N, K, epilogue, (hipStream_t)stream));
    return LOCO_OK;
}

size_t loco_decoder_attention_scratch_bytes(int32_t B, int32_t Sq, int32_t Tk) {
    return B > 0 && Sq > 0 && Tk > 0 ? dec_attention_scratch_bytes(B, Sq, Tk) : 0;
}

int loco_op_decoder_attention(const float* q, const float* k, const float* v, const int32_t* key_counts, float* out, int32_t B, int32_t Sq,
                              int32_t Tk, int32_t causal, int32_t causal_offset, float scale, void* scratch, size_t scratch_bytes, void* stream) {
    if (!q || !k || !v || !out || B <= 0 || Sq <= 0 || Tk <= 0) return fail(LOCO_E_INVALID, "loco_op_decoder_attention: null / non-positive argument");
    if (scratch_bytes < dec_attention_scratch_bytes(B, Sq, Tk))
        return fail(LOCO_E_WORKSPACE, "loco_op_decoder_attention: scratch %zu < %zu bytes", scratch_bytes, dec_attention_scratch_bytes(B, Sq, Tk));
    HIP_TRY(launch_dec_attention(q, kHidden, (long)Sq * kHidden, k, kHidden, (long)Tk * kHidden, v, kHidden, (long)Tk * kHidden, key_counts, out, kHidden,
                                 (long)Sq * kHidden, B, Sq, Tk, causal, causal_offset, scale, static_cast<float*>(scratch), (hipStream_t)stream));
    return LOCO_OK;
}

// ---- the decode step's and the slot pool's forms of the two kernels as operators (tests/test_gpu_decoder_contract.py) ----
int loco_op_skinny_gemm_split(const float* A, int64_t lda, const float* Wt, int64_t ldw, const float* bias, float* C, int64_t ldc, float* C2,
                              int64_t ldc2, const int32_t* c2_rows, int64_t c2_row_stride, int32_t nsplit, int32_t M, int32_t N, int32_t K,
                              void* stream) {
    const char* fn = "loco_op_skinny_gemm_split";
    if (!A || !Wt || !C || !C2) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (M <= 0 || N <= 0 || K <= 0 || K % 256 != 0) return fail(LOCO_E_INVALID, "%s: M = %d, N = %d, K = %d: all positive, K a multiple of 256", fn, M, N, K);
    if (M > kSkinnyMaxM) return fail(LOCO_E_INVALID, "%s: M = %d exceeds the limit of %d rows", fn, M, kSkinnyMaxM);
    if (nsplit < 0 || nsplit > N) return fail(LOCO_E_INVALID, "%s: nsplit = %d is outside 0 .. N = %d", fn, nsplit, N);
    if (lda < K || ldw < K || ((lda | ldw) & 3)) return fail(LOCO_E_INVALID, "%s: lda and ldw must be >= K and multiples of 4 floats", fn);
    if (ldc < nsplit || (!c2_rows && ldc2 < N - nsplit) || (c2_rows && c2_row_stride < N - nsplit))
        return fail(LOCO_E_INVALID, "%s: a destination row is shorter than its %d / %d columns", fn, nsplit, N - nsplit);
    if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Wt)) & 15) return fail(LOCO_E_INVALID, "%s: A and W must be 16-byte aligned", fn);
    if (!c2_rows)
        HIP_TRY(launch_skinny_gemm(A, (long)lda, Wt, (long)ldw, bias, nullptr, 0, C, (long)ldc, C2, (long)ldc2, nsplit, M, N, K, kEpiNone, (hipStream_t)stream));
    else
        HIP_TRY(launch_skinny_gemm_rows(A, (long)lda, Wt, (long)ldw, bias, C, (long)ldc, C2, (long)ldc2, c2_rows, (long)c2_row_stride, nsplit, M, N, K,
                                        (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_decoder_attention_strided(const float* q, int64_t ldq, int64_t sq, const float* k, int64_t ldk, int64_t sk, const float* v, int64_t ldv,
                                      int64_t sv, const int32_t* key_counts, float* out, int64_t ldo, int64_t so, int32_t B, int32_t Sq, int32_t Tk,
                                      int32_t causal, int32_t causal_offset, float scale, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "loco_op_decoder_attention_strided";
    if (!q || !k || !v || !out || B <= 0 || Sq <= 0 || Tk <= 0) return fail(LOCO_E_INVALID, "%s: null / non-positive argument", fn);
    if (ldq < kHidden || ldk < kHidden || ldv < kHidden || ldo < kHidden || ((ldq | ldk | sq | sk) & 3))
        return fail(LOCO_E_INVALID, "%s: row strides must be >= 768 floats, those of q and k and their clip strides multiples of 4 floats", fn);
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return fail(LOCO_E_INVALID, "%s: q and k must be 16-byte aligned", fn);
    if (scratch_bytes < dec_attention_scratch_bytes(B, Sq, Tk) || (!scratch && dec_attention_scratch_bytes(B, Sq, Tk) > 0))
        return fail(LOCO_E_WORKSPACE, "%s: scratch %zu < %zu bytes", fn, scratch ? scratch_bytes : (size_t)0, dec_attention_scratch_bytes(B, Sq, Tk));
    HIP_TRY(launch_dec_attention(q, (long)ldq, (long)sq, k, (long)ldk, (long)sk, v, (long)ldv, (long)sv, key_counts, out, (long)ldo, (long)so, B, Sq, Tk,
                                 causal, causal_offset, scale, static_cast<float*>(scratch), (hipStream_t)stream));
    return LOCO_OK;
}

size_t loco_decoder_pool_attention_scratch_bytes(int32_t slots, int32_t Tk_bound) {
    return slots > 0 && Tk_bound > 0 ? dec_pool_attention_scratch_bytes(slots, Tk_bound) : 0;
}

int loco_op_decoder_pool_attention(const float* q, const float* k, int64_t ldk, int64_t sk, const float* v, const int32_t* key_counts, float* out,
                                   int32_t slots, int32_t Tk_bound, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "loco_op_decoder_pool_attention";
    if (!q || !k || !v || !key_counts || !out || !scratch) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (slots <= 0 || slots > kSkinnyMaxM || Tk_bound <= 0)
        return fail(LOCO_E_INVALID, "%s: slots = %d must be 1 .. %d, Tk_bound = %d positive", fn, slots, kSkinnyMaxM, Tk_bound);
    if (ldk < kHidden || ((ldk | sk) & 3)) return fail(LOCO_E_INVALID, "%s: ldk must be >= 768 floats, ldk and sk multiples of 4 floats", fn);
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return fail(LOCO_E_INVALID, "%s: q and k must be 16-byte aligned", fn);
    if (scratch_bytes < dec_pool_attention_scratch_bytes(slots, Tk_bound))
        return fail(LOCO_E_WORKSPACE, "%s: scratch %zu < %zu bytes", fn, scratch_bytes, dec_pool_attention_scratch_bytes(slots, Tk_bound));
    HIP_TRY(launch_dec_pool_attention(q, k, (long)ldk, (long)sk, v, key_counts, out, slots, Tk_bound, static_cast<float*>(scratch), (hipStream_t)stream));
    return LOCO_OK;
}

// ---- decoder attention probabilities and the DTW as operators (decoder_probs.hip) ----
int loco_op_decoder_attention_probs(const float* q, const float* k, const int32_t* key_counts, float* P, int32_t B, int32_t Sq, int32_t Tk,
                                    int32_t causal, int64_t ldq, int64_t sq, int64_t ldk, int64_t sk, float scale, void* stream) {
    const char* fn = "loco_op_decoder_attention_probs";
    if (!q || !k || !P || B <= 0 || Sq <= 0 || Tk <= 0) return fail(LOCO_E_INVALID, "%s: null / non-positive argument", fn);
    if (ldq < kHidden || ldk < kHidden || ((ldq | ldk | sq | sk) & 3))
        return fail(LOCO_E_INVALID, "%s: row strides must be >= 768 floats, every stride a multiple of 4 floats", fn);
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return fail(LOCO_E_INVALID, "%s: q and k must be 16-byte aligned", fn);
    HIP_TRY(launch_dec_attention_probs(q, (long)ldq, (long)sq, k, (long)ldk, (long)sk, key_counts, P, B, Sq, Tk, causal, scale, (hipStream_t)stream));
    return LOCO_OK;
}

size_t loco_dtw_align_workspace_bytes(int32_t B, int32_t S, int32_t T) { return B > 0 && S > 0 && T > 0 ? (size_t)B * S * T : 0; }

int loco_op_dtw_align(const float* A, int64_t ld, const int32_t* n, const int32_t* frames, int32_t B, int32_t S, int32_t T, int32_t* start,
                      int32_t* end, void* workspace, void* stream) {
    const char* fn = "loco_op_dtw_align";
    if (!A || !n || !start || !end || !workspace) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (B <= 0 || S <= 0 || T <= 0) return fail(LOCO_E_INVALID, "%s: B, S and T must be positive", fn);
    if (S > kDecAlignMaxTokens) return fail(LOCO_E_INVALID, "%s: %d tokens exceed the limit of %d rows (max_text_positions)", fn, S, kDecAlignMaxTokens);
    if (ld < T) return fail(LOCO_E_INVALID, "%s: row stride ld = %lld < T = %d", fn, (long long)ld, T);
    HIP_TRY(launch_dtw_align(A, (long)ld, n, frames, B, S, T, start, end, static_cast<unsigned char*>(workspace), (hipStream_t)stream));
    return LOCO_OK;
}

// ---- decoder scores (decoder_score.hip) ----
int loco_decoder_score(const float* logits, int64_t ld, const int32_t* targets, int32_t B, int32_t S, int32_t V, int32_t ignore_index,
                       float* token_logprobs, int32_t* chosen, float* seq_logprob, int32_t* seq_count, float* loss, void* stream) {
    if (!logits || !token_logprobs) return fail(LOCO_E_INVALID, "loco_decoder_score: null logits or token_logprobs");
    if (B < 1 || S < 1 || V < 1) return fail(LOCO_E_INVALID, "loco_decoder_score: B = %d, S = %d, V = %d must all be >= 1", B, S, V);
    if (ld < V) return fail(LOCO_E_INVALID, "loco_decoder_score: row stride ld = %lld < V = %d", (long long)ld, V);
    if ((long)B * S > 0x7fffffffL) return fail(LOCO_E_INVALID, "loco_decoder_score: B * S = %ld rows exceed 2^31 - 1", (long)B * S);
    HIP_TRY(launch_token_logprob(logits, (long)ld, targets, (long)B * S, V, ignore_index, token_logprobs, chosen, (hipStream_t)stream));
    if (seq_logprob || seq_count || loss)
        HIP_TRY(launch_score_reduce(token_logprobs, targets, B, S, ignore_index, seq_logprob, seq_count, loss, (hipStream_t)stream));
    return LOCO_OK;
}
