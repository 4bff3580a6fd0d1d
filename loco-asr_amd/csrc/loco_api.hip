// C ABI (include/loco_asr.h) and the host-side orchestration of the encoder forward.
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

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/loco_asr.h"
#include "loco_kernels.h"

using namespace loco;

namespace {

thread_local std::string g_err;

}  // namespace

namespace loco {
int api_fail(int code, const char* fmt, ...) {  // declared in loco_kernels.h: lm_api.hip reports through the same string
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace loco

namespace {

constexpr auto& fail = loco::api_fail;

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(LOCO_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

const int kConvK[7] = {10, 3, 3, 3, 3, 2, 2};
const int kConvS[7] = {5, 2, 2, 2, 2, 2, 2};

struct SplitW {  // fp16 hi/lo planes of one GEMM weight (precision mode f16x3), holding W * 2^k; inv_scale = 2^-k
    _Float16* hi = nullptr;
    _Float16* lo = nullptr;
    float inv_scale = 1.0f;
};

// Checkpoint tensors the forward reads as loaded (loco_encoder::raw) are bound here by loco_finalize_weights, so that no forward
// looks a name up.  loco_set_weight reuses a key's device buffer once allocated, so a bound pointer cannot go stale.
struct WB {  // "<prefix>weight" and "<prefix>bias": a Linear's W and b, a LayerNorm's (or the GroupNorm's) gamma and beta
    const float *w = nullptr, *b = nullptr;
};
struct LayerW {
    float* wqkv = nullptr;  // [2304,768], q rows pre-scaled by 1/8
    float* bqkv = nullptr;  // [2304]
    SplitW sqkv, so, s1, s2;
    WB out_proj, layer_norm, ffn_in, ffn_out, final_layer_norm;  // ffn_in / ffn_out: feed_forward.intermediate_dense / output_dense
};
struct StemW {  // the prenet's tensors (bound for a handle with the speech prenet only), the encoder's input LayerNorm and pe_k
    WB conv0_norm, proj_norm, proj;  // feature_encoder.conv_layers.0.layer_norm, feature_projection.layer_norm / .projection
    const float* pos_b = nullptr;    // pos_conv_embed.conv.bias
    WB layer_norm;                   // wrapped_encoder.layer_norm
    const float* pe_k = nullptr;     // wrapped_encoder.embed_positions.pe_k [320,64]
};

// Text decoder (SpeechT5DecoderWithTextPrenet + SpeechT5TextDecoderPostnet): optional, bound by loco_finalize_weights when the handle
// was given decoder tensors.  Everything is fp32 in every precision mode (rows are few; the step is bandwidth-bound).
struct DecLayerW {
    float* wqkv = nullptr;  // self-attention [2304,768], q rows pre-scaled by 1/8
    float* bqkv = nullptr;
    float* wcq = nullptr;   // cross-attention q [768,768] pre-scaled by 1/8
    float* bcq = nullptr;
    WB self_out, self_ln, cross_out, cross_ln, ffn_in, ffn_out, final_ln;
};
struct DecoderW {
    int layers = 0;         // from the keys
    bool ready = false;
    std::vector<DecLayerW> L;
    float* wckv = nullptr;  // cross-attention k|v of every layer, [layers * 1536, 768]: one product per utterance
    float* bckv = nullptr;
    const float* embed = nullptr;
    const float* lm_head = nullptr;
    int vocab = 0;
    float* pos_tab = nullptr;  // [pos_rows, 768], HF SpeechT5SinusoidalPositionalEmbedding (padding row 1 = 0)
    int pos_rows = 0;
    bool pos_user = false;
    int32_t* host_state = nullptr;  // pinned: loco_decoder_generate reads the device's "rows still open" word through it
};
constexpr int kDecMaxPositions = 450;  // SpeechT5Config.max_text_positions; HF's table has max_text_positions + pad_token_id + 1 = 452 rows

// Profiling buckets, named after the kernel that runs in them (the two precision modes have their own attention and
// positional-conv buckets: the f16x3 positional conv IS a gemm_f16x3_dma_kernel launch, but keeps a bucket of its own because
// its shape -- N = 48, K = 6144, halo layout -- has little in common with the projection GEMMs).
enum KernelId { K_GEMM = 0, K_ATTN, K_LN, K_CONV0, K_POSCONV, K_FRAMES, K_COPY, K_GEMM_SPLIT, K_ATTN_SPLIT, K_POSCONV_SPLIT, K_ATTN_PROBS, K_COUNT };
const char* const kKernelNames[K_COUNT] = {"gemm_f32",     "attention_f32", "layernorm",       "conv0_gn_gelu",
                                           "pos_conv_f32", "frame_counts",  "copy",            "gemm_f16x3",
                                           "attention_f16x3", "pos_conv_f16x3_gemm", "attention_probs"};

struct ProfRec {
    hipEvent_t a, b;
    int kid;
    double flops, bytes;
};

// Status block of ONE forward (include/loco_asr.h, loco_status_bytes): host memory, caller-owned for loco_forward_async, the
// handle's own pinned block for loco_forward.  The host part is filled while the forward is enqueued; `words` is the target of the
// device-to-host copy that follows the forward on its stream.
constexpr uint32_t kStatusMagic = 0x53434f4cu;  // "LOCS"
constexpr int kMaxPackClips = 512;              // clips per loco_forward_packed
struct StatusBlock {
    uint32_t magic;
    int32_t precision;                        // arithmetic mode of the forward this block describes
    int32_t used;                             // stages filled
    int32_t layer[kRangeMaxStages];
    const char* names[kRangeMaxStages];       // static strings of this library
    char msg[384];                            // non-empty: a range verdict known on the host (weights outside the planes' range)
    float words[kRangeMaxStages * kRangeShards];
    // loco_forward_packed: per clip, the conv-layer-0 and the encoder frame counts of its OWN reference batch's padded length
    // ([0, B): conv0 frames, [B, 2B): encoder frames, [2B, 3B): valid frames when the caller gave valid_len instead of a mask).
    // Staged here because the block is host memory the caller keeps alive (and pinned) until the stream has completed the forward:
    // the source of the host-to-device copy that opens the forward.
    int32_t clip_tab[3 * kMaxPackClips];
};
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

}  // namespace

struct loco_encoder {
    loco_config cfg;
    int device = 0;
    std::map<std::string, float*> raw;  // device copies as loaded, HF names
    std::map<std::string, std::vector<int64_t>> expected;
    bool finalized = false;
    // prepared
    float* conv_w[7] = {nullptr};  // [512, k*512] tap-major (layer 0 stays [512,10])
    float* pos_w = nullptr;        // [16][128][48][48]
    SplitW conv_s[7];              // split copies of conv_w[1..6]
    SplitW proj_s;                 // feature projection
    SplitW pe_s;                   // relative-position table pe_k [320,64]
    SplitW posg_s;                 // positional conv weight as the GEMM's W: [16][48][128*48]
    int precision = 1;             // 0 = exact fp32 MFMA, 1 = fp16 x3 split MFMA (default), 2 = f16x2 (weights rounded to fp16; opt-in)
    std::vector<LayerW> layers;
    StemW stem;
    // published with release stores (table first, then its row count), read with acquire loads: a forward on another host thread
    // that sees the new row count also sees the new, longer table (ensure_sin_rows; loco_forward_async allows concurrent callers)
    std::atomic<float*> sin_tab{nullptr};
    std::atomic<int> sin_rows{0};
    bool sin_user = false;
    std::mutex sin_mu;            // growth of the sinusoid table (ensure_sin_rows)
    std::vector<float*> retired;  // tables replaced while forwards may still have been reading them: freed at loco_destroy
    // taps
    float *tap_conv = nullptr, *tap_proj = nullptr, *tap_prenet = nullptr;
    // attention probabilities (loco_set_attention_outputs): one fp32 [B,12,T,T] buffer per layer, or empty
    std::vector<float*> attn_probs;
    // text front end (SpeechT5TextEncoderPrenet): optional; a handle may carry the speech prenet, the text prenet or both
    float* text_embed = nullptr;  // [text_vocab, 768]
    int text_vocab = 0;
    float* text_alpha = nullptr;  // [1]
    float* text_pe = nullptr;     // [text_pe_rows, 768]
    int text_pe_rows = 0;
    bool speech_ready = false;    // set by loco_finalize_weights when the speech prenet weights were supplied
    DecoderW dec;                 // text decoder (optional)
    // decoder pools that hold slots which sample: (workspace, bit r = slot r draws).  On the host because loco_decoder_pool_admit and
    // loco_decoder_pool_step enqueue what they always did: neither can mark a slot on the device.  Single caller, as the pool itself.
    std::vector<std::pair<const void*, unsigned long long>> pool_sampled;
    std::map<std::string, std::vector<int64_t>> dec_shapes;  // shapes of the decoder tensors as loaded (the vocabulary is theirs)
    // concurrency inside one forward: a batch may run as two half-batches on two streams (loco_set_streams).  The side stream and
    // its events are created on first use under side_mu; forwards in flight together serialise their second halves on it.
    int streams = 2;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::mutex side_mu;
    // range tracking of the fp16-plane activations (loco_kernels.h, range_commit): one status word x 8 shards per stage, in the
    // workspace of each forward; `own` is the status block of the forwards enqueued through loco_forward (pinned host memory)
    StatusBlock* own = nullptr;
    float* absmax_dev = nullptr;  // one float, weight preparation
    bool debug_nonfinite = false;                 // LOCO_DEBUG_NONFINITE=1 at loco_create (dbg_check)
    unsigned long long* debug_counter = nullptr;  // two words, device
    int range_policy = 1;         // loco_forward_checked: 1 = re-run out-of-range batches on the exact-fp32 kernels, 0 = report
    std::string range_static;     // non-empty: a weight-determined plane tensor (a LayerNorm output) leaves the range
    // profiling
    bool profiling = false;
    int profile_only = -1;  // >= 0: only launches of this kernel bucket are bracketed (loco_set_profiling_filter)
    std::vector<ProfRec> recs;
    size_t recs_used = 0;
    loco_kernel_stat stats[K_COUNT];
};

namespace {

void build_expected(loco_encoder* e) {
    auto& x = e->expected;
    const int64_t H = e->cfg.hidden, C = e->cfg.conv_dim, F = e->cfg.ffn;
    const std::string p = "prenet.";
    x[p + "masked_spec_embed"] = {H};
    for (int i = 0; i < 7; ++i)
        x[p + "feature_encoder.conv_layers." + std::to_string(i) + ".conv.weight"] = {C, i == 0 ? 1 : C, kConvK[i]};
    x[p + "feature_encoder.conv_layers.0.layer_norm.weight"] = {C};
    x[p + "feature_encoder.conv_layers.0.layer_norm.bias"] = {C};
    x[p + "feature_projection.layer_norm.weight"] = {C};
    x[p + "feature_projection.layer_norm.bias"] = {C};
    x[p + "feature_projection.projection.weight"] = {H, C};
    x[p + "feature_projection.projection.bias"] = {H};
    x[p + "pos_conv_embed.conv.bias"] = {H};
    x[p + "pos_conv_embed.conv.parametrizations.weight.original0"] = {1, 1, e->cfg.pos_conv_kernel};
    x[p + "pos_conv_embed.conv.parametrizations.weight.original1"] = {H, H / e->cfg.pos_conv_groups, e->cfg.pos_conv_kernel};
    const std::string w = "wrapped_encoder.";
    x[w + "layer_norm.weight"] = {H};
    x[w + "layer_norm.bias"] = {H};
    x[w + "embed_positions.pe_k.weight"] = {2 * e->cfg.rel_max, H / e->cfg.heads};
    for (int l = 0; l < e->cfg.layers; ++l) {
        const std::string b = w + "layers." + std::to_string(l) + ".";
        for (const char* pr : {"q_proj", "k_proj", "v_proj", "out_proj"}) {
            x[b + "attention." + pr + ".weight"] = {H, H};
            x[b + "attention." + pr + ".bias"] = {H};
        }
        for (const char* ln : {"layer_norm", "final_layer_norm"}) {
            x[b + ln + ".weight"] = {H};
            x[b + ln + ".bias"] = {H};
        }
        x[b + "feed_forward.intermediate_dense.weight"] = {F, H};
        x[b + "feed_forward.intermediate_dense.bias"] = {F};
        x[b + "feed_forward.output_dense.weight"] = {H, F};
        x[b + "feed_forward.output_dense.bias"] = {H};
    }
}

bool optional_key(const std::string& k) { return k == "prenet.masked_spec_embed"; }

// Decoder tensors (HF names below "speecht5.", as the encoder's): the shape a key must have, or false for a key that is none.
// The vocabulary size is taken from the tensor ([V,768], V >= 3: the special tokens 0..2 exist).
const char* const kDecLayerLinear[] = {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj",
                                       "encoder_attn.q_proj", "encoder_attn.k_proj", "encoder_attn.v_proj", "encoder_attn.out_proj"};
const char* const kDecLayerNorm[] = {"self_attn_layer_norm", "encoder_attn_layer_norm", "final_layer_norm"};
const std::string kDecEmbedKey = "decoder.prenet.embed_tokens.weight", kDecHeadKey = "text_decoder_postnet.lm_head.weight",
                  kDecLayerPrefix = "decoder.wrapped_decoder.layers.";

std::vector<std::pair<std::string, std::vector<int64_t>>> decoder_layer_keys(int l) {
    std::vector<std::pair<std::string, std::vector<int64_t>>> out;
    const std::string b = kDecLayerPrefix + std::to_string(l) + ".";
    for (const char* pr : kDecLayerLinear) {
        out.push_back({b + pr + ".weight", {kHidden, kHidden}});
        out.push_back({b + pr + ".bias", {kHidden}});
    }
    for (const char* ln : kDecLayerNorm) {
        out.push_back({b + ln + ".weight", {kHidden}});
        out.push_back({b + ln + ".bias", {kHidden}});
    }
    out.push_back({b + "feed_forward.intermediate_dense.weight", {kFfn, kHidden}});
    out.push_back({b + "feed_forward.intermediate_dense.bias", {kFfn}});
    out.push_back({b + "feed_forward.output_dense.weight", {kHidden, kFfn}});
    out.push_back({b + "feed_forward.output_dense.bias", {kHidden}});
    return out;
}

int decoder_layer_of(const std::string& k) {  // -1: not a decoder layer key
    if (k.rfind(kDecLayerPrefix, 0) != 0) return -1;
    size_t i = kDecLayerPrefix.size(), j = i;
    while (j < k.size() && k[j] >= '0' && k[j] <= '9') ++j;
    if (j == i || j - i > 2 || j >= k.size() || k[j] != '.') return -1;
    return atoi(k.substr(i, j - i).c_str());
}

bool decoder_key_shape(const std::string& k, const std::vector<int64_t>& got, std::vector<int64_t>& want) {
    if (k == kDecEmbedKey || k == kDecHeadKey) {
        want = {got.size() == 2 && got[0] >= 3 ? got[0] : 81, kHidden};
        return true;
    }
    const int l = decoder_layer_of(k);
    if (l < 0) return false;
    for (auto& kv : decoder_layer_keys(l))
        if (kv.first == k) {
            want = kv.second;
            return true;
        }
    return false;
}

// decoder layer count of the tensors loaded so far (0: none), and whether any decoder tensor was given at all
int decoder_layers_loaded(const loco_encoder* e, bool* any) {
    int layers = 0;
    bool seen = false;
    for (auto& kv : e->raw) {
        const int l = decoder_layer_of(kv.first);
        if (l >= 0) layers = l + 1 > layers ? l + 1 : layers;
        seen = seen || l >= 0 || kv.first == kDecEmbedKey || kv.first == kDecHeadKey;
    }
    if (any) *any = seen;
    return layers;
}

// Decoder tensors still missing on a handle that was given SOME of them (it must then have them all; one of the tied embedding /
// lm_head pair suffices); 0 for a handle without any decoder tensor.  Names are appended to *names, comma separated.
int decoder_missing(const loco_encoder* e, std::string* names) {
    bool any = false;
    const int layers = decoder_layers_loaded(e, &any);
    if (!any) return 0;
    int missing = 0;
    auto need = [&](const std::string& k) {
        if (e->raw.count(k)) return;
        ++missing;
        if (names) *names += (names->empty() ? "" : ",") + k;
    };
    if (!e->raw.count(kDecEmbedKey) && !e->raw.count(kDecHeadKey)) need(kDecEmbedKey);
    if (layers == 0) need(kDecLayerPrefix + "0.self_attn.q_proj.weight");
    for (int l = 0; l < layers; ++l)
        for (auto& kv : decoder_layer_keys(l)) need(kv.first);
    return missing;
}

std::string canonical_key(const char* key) {
    std::string k(key);
    const std::string a = "pos_conv_embed.conv.weight_g", b = "pos_conv_embed.conv.weight_v";
    size_t pos;
    if ((pos = k.find(a)) != std::string::npos && pos + a.size() == k.size())
        k.replace(pos, a.size(), "pos_conv_embed.conv.parametrizations.weight.original0");
    else if ((pos = k.find(b)) != std::string::npos && pos + b.size() == k.size())
        k.replace(pos, b.size(), "pos_conv_embed.conv.parametrizations.weight.original1");
    return k;
}

const float* W(const loco_encoder* e, const std::string& k) { return e->raw.at(k); }
WB weight_bias(const loco_encoder* e, const std::string& prefix) { return {W(e, prefix + "weight"), W(e, prefix + "bias")}; }

size_t align_up(size_t n) { return (n + 255) & ~size_t(255); }

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

// ---- profiling brackets -----------------------------------------------------------------------------
struct Bracket {
    loco_encoder* e;
    hipStream_t s;
    ProfRec* rec = nullptr;
    Bracket(loco_encoder* enc, hipStream_t st, int kid, double flops, double bytes) : e(enc), s(st) {
        if (!e->profiling || (e->profile_only >= 0 && e->profile_only != kid)) return;
        if (e->recs_used == e->recs.size()) {
            ProfRec r{};
            if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
            e->recs.push_back(r);
        }
        rec = &e->recs[e->recs_used++];
        rec->kid = kid;
        rec->flops = flops;
        rec->bytes = bytes;
        (void)hipEventRecord(rec->a, s);
    }
    ~Bracket() {
        if (rec) (void)hipEventRecord(rec->b, s);
    }
};

// algorithmic FLOPs and fp32 bytes of a (batched) GEMM, as the profiling brackets report them
double gemm_flops(int M, int N, int K, int nb1, int nb2) { return 2.0 * M * (double)N * K * ((double)nb1 * nb2); }
double gemm_bytes(int M, int N, int K, int nb1, int nb2, int epi) {
    const double nb = (double)nb1 * nb2;
    return 4.0 * (nb * ((double)M * K + (double)M * N * (epi == kEpiResidual ? 2 : 1)) + (double)N * K);
}

int run_gemm(loco_encoder* e, hipStream_t s, const float* A, long lda, const float* Wt, long ldw, const float* bias,
             const float* R, long ldr, float* C, long ldc, int M, int N, int K, int epi, int nb1 = 1, int nb2 = 1,
             long sA1 = 0, long sA2 = 0, long sC1 = 0, long sC2 = 0) {
    GemmArgs a{A, Wt, bias, R, C, M, N, K, lda, ldw, ldc, ldr, nb1, nb2, sA1, sA2, sC1, sC2, epi};
    Bracket br(e, s, K_GEMM, gemm_flops(M, N, K, nb1, nb2), gemm_bytes(M, N, K, nb1, nb2, epi));
    HIP_TRY(launch_gemm(a, s));
    return LOCO_OK;
}

int run_ln(loco_encoder* e, hipStream_t s, const float* x, const float* g, const float* b, float* y, long rows, int dim,
           _Float16* yhi = nullptr, _Float16* ylo = nullptr, float* nonfinite_slot = nullptr) {
    Bracket br(e, s, K_LN, 8.0 * rows * dim, (y && yhi ? 12.0 : 8.0) * rows * dim);
    HIP_TRY(launch_layernorm(x, g, b, y, rows, dim, e->cfg.ln_eps, s, yhi, ylo, nonfinite_slot));
    return LOCO_OK;
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

int absmax_host(loco_encoder* e, const float* src, size_t n, hipStream_t s, float& out) {
    HIP_TRY(hipMemsetAsync(e->absmax_dev, 0, sizeof(float), s));
    HIP_TRY(launch_absmax(src, (long)n, e->absmax_dev, s));
    HIP_TRY(hipMemcpyAsync(&out, e->absmax_dev, sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return LOCO_OK;
}

// Weight planes: W * 2^k with k such that max|W| lands in [2^13, 2^14) -- the largest element then sits two binades under
// fp16's maximum and elements down to 2^-27 of it still have a normal fp16 lo part, whatever the tensor's absolute level
// (a checkpoint with weights of 1e-6 or of 1e+3 is represented exactly as well as one with weights of 0.03).  The GEMM
// multiplies its accumulator by inv_scale = 2^-k (exact).  One tiny reduction + one host read per tensor, at load time only.
int make_split(loco_encoder* e, SplitW& w, const float* src, size_t n, hipStream_t s) {
    if (!w.hi) HIP_TRY(hipMalloc(&w.hi, n * sizeof(_Float16)));
    if (!w.lo) HIP_TRY(hipMalloc(&w.lo, n * sizeof(_Float16)));
    float amax = 0.f;
    if (int rc = absmax_host(e, src, n, s, amax)) return rc;
    int k = 0;
    if (amax > 0.f && amax < INFINITY) {
        int ex = 0;
        (void)frexpf(amax, &ex);  // amax = f * 2^ex, f in [0.5, 1)  ->  amax * 2^(14 - ex) in [2^13, 2^14)
        k = 14 - ex;
        k = k > 100 ? 100 : (k < -100 ? -100 : k);
    }
    w.inv_scale = ldexpf(1.0f, -k);
    HIP_TRY(launch_split_f16(src, w.hi, w.lo, (long)n, s, ldexpf(1.0f, k)));
    return LOCO_OK;
}

constexpr float kRangeHi = 65504.0f;   // fp16 maximum: hi = fp16(x) is inf from 65520 on
constexpr float kRangeLo = 0.015625f;  // 2^-6: a plane tensor whose LARGEST element is below this has lost fp32-class accuracy

// Plane tensors whose range follows from the weights: y = x_hat * gamma + beta with sum(x_hat^2) <= D gives
// |y| <= sqrt(D) max|gamma| + max|beta| (LayerNorm over D channels), and a unit-variance x_hat puts the tensor's largest element near max(max|gamma|, max|beta|).  The attention
// context is a convex combination of V rows, tracked with q|k|v.  Checked once per weight load; nothing is measured at run time.
int static_range_check(loco_encoder* e, const std::string& ln_prefix, int dim, hipStream_t s) {
    float g = 0.f, b = 0.f;
    int rc = absmax_host(e, W(e, ln_prefix + "weight"), (size_t)dim, s, g);
    if (!rc) rc = absmax_host(e, W(e, ln_prefix + "bias"), (size_t)dim, s, b);
    if (rc) return rc;
    const float hi = sqrtf((float)dim) * g + b, lo = fmaxf(g, b);
    if (e->range_static.empty() && (!(hi < kRangeHi) || lo < kRangeLo)) {
        char msg[320];
        snprintf(msg, sizeof msg, "activation range: the output of '%s*' (max|weight| = %.6g, max|bias| = %.6g) is %s the range precision mode "
                 "f16x3 represents to fp32 class (%g <= max|x| < %g)", ln_prefix.c_str(), (double)g, (double)b,
                 !(hi < kRangeHi) ? "not bounded inside" : "below", (double)kRangeLo, (double)kRangeHi);
        e->range_static = msg;
    }
    return LOCO_OK;
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

int run_copy(loco_encoder* e, hipStream_t s, float* dst, const float* src, size_t n) {
    Bracket br(e, s, K_COPY, 0.0, 8.0 * n);
    HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return LOCO_OK;
}

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
    int rc;
    // ---- feature encoder (HF :484-494)
    if ((rc = run_conv0(e, s, p, wav, bf, bf.bufA, nullptr, nullptr, nullptr))) return rc;
    float* cin = bf.bufA;
    float* cout = bf.bufB;
    for (int i = 1; i < 7; ++i) {
        const long Tin = p.Tc[i - 1], Tout = p.Tc[i];
        rc = run_gemm(e, s, cin, (long)kConvS[i] * kConvDim, e->conv_w[i], (long)kConvK[i] * kConvDim, nullptr, nullptr, 0,
                      cout, kConvDim, (int)Tout, kConvDim, kConvK[i] * kConvDim, kEpiGelu, B, 1, Tin * kConvDim, 0,
                      Tout * kConvDim, 0);
        if (rc) return rc;
        std::swap(cin, cout);
    }
    float* feats = cin;  // [M,512]
    if (e->tap_conv && (rc = run_copy(e, s, e->tap_conv, feats, (size_t)M * kConvDim))) return rc;

    // ---- feature projection (HF :498-510): LayerNorm(512) in place, then Linear(512,768)
    if ((rc = run_ln(e, s, feats, sw.proj_norm.w, sw.proj_norm.b, feats, M, kConvDim))) return rc;
    if ((rc = run_gemm(e, s, feats, kConvDim, sw.proj.w, kConvDim, sw.proj.b, nullptr, 0, bf.x1, kHidden, (int)M, kHidden, kConvDim,
                       kEpiNone)))
        return rc;
    if (e->tap_proj && (rc = run_copy(e, s, e->tap_proj, bf.x1, (size_t)M * kHidden))) return rc;

    // ---- positional conv + sinusoid (HF :555-564)
    {
        Bracket br(e, s, K_POSCONV, 2.0 * M * (double)kHidden * kPosCg * kPosK, 8.0 * M * kHidden);
        HIP_TRY(launch_pos_conv(bf.x1, e->pos_w, sw.pos_b, bf.sin_tab, bf.frames_or_null, bf.x0, B, (int)p.T, s, bf.rows_clip));
    }
    if (e->tap_prenet && (rc = run_copy(e, s, e->tap_prenet, bf.x0, (size_t)M * kHidden))) return rc;
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
    int rc;
    float *x0 = bf.x0, *x1 = bf.x1, *tmp = bf.tmp, *ctx = bf.ctx, *qkv = bf.qkv, *qp = bf.qp, *ffn = bf.ffn;
    if ((rc = run_ln(e, s, x0, e->stem.layer_norm.w, e->stem.layer_norm.b, x0, M, kHidden))) return rc;
    const int nl = e->cfg.layers;
    for (int l = 0; l < nl; ++l) {
        if (hidden_states && hidden_states[l] && (rc = run_copy(e, s, hidden_states[l], x0, (size_t)M * kHidden))) return rc;
        const LayerW& lw = e->layers[l];
        // fused q|k|v projection, q pre-scaled (HF :891,911-914)
        if ((rc = run_gemm(e, s, x0, kHidden, lw.wqkv, kHidden, lw.bqkv, nullptr, 0, qkv, kQkv, (int)M, kQkv, kHidden, kEpiNone)))
            return rc;
        // Qp[b,h] = q_scaled[b,:,h,:] pe_k^T  -> [B,12,T,320]
        if ((rc = run_gemm(e, s, qkv, kQkv, e->stem.pe_k, kHeadDim, nullptr, nullptr, 0, qp, kRelN, T, kRelN, kHeadDim, kEpiNone, B,
                           kHeads, (long)T * kQkv, kHeadDim, (long)kHeads * T * kRelN, (long)T * kRelN)))
            return rc;
        {
            const double tt = (double)T * T;
            Bracket br(e, s, K_ATTN, 4.0 * B * kHeads * tt * kHeadDim, 4.0 * (M * (double)(kQkv + kHidden) + M * (double)kHeads * kRelN));
            HIP_TRY(launch_attention(qkv, qp, bf.frames_or_null, ctx, B, T, s));
        }
        if ((rc = run_attention_probs(e, s, qkv, nullptr, nullptr, nullptr, nullptr, qp, bf.frames_or_null, l, B, T))) return rc;
        // out_proj + residual (HF :984,1056), LayerNorm (HF :1058)
        if ((rc = run_gemm(e, s, ctx, kHidden, lw.out_proj.w, kHidden, lw.out_proj.b, x0, kHidden, tmp, kHidden, (int)M, kHidden, kHidden,
                           kEpiResidual)))
            return rc;
        if ((rc = run_ln(e, s, tmp, lw.layer_norm.w, lw.layer_norm.b, x1, M, kHidden))) return rc;
        // FFN (HF :1003-1010) + residual + final LayerNorm (HF :1059-1060)
        if ((rc = run_gemm(e, s, x1, kHidden, lw.ffn_in.w, kHidden, lw.ffn_in.b, nullptr, 0, ffn, e->cfg.ffn, (int)M, e->cfg.ffn, kHidden,
                           kEpiGelu)))
            return rc;
        if ((rc = run_gemm(e, s, ffn, e->cfg.ffn, lw.ffn_out.w, e->cfg.ffn, lw.ffn_out.b, x1, kHidden, tmp, kHidden, (int)M, kHidden,
                           e->cfg.ffn, kEpiResidual)))
            return rc;
        float* dst = (l == nl - 1) ? out : x0;
        if ((rc = run_ln(e, s, tmp, lw.final_layer_norm.w, lw.final_layer_norm.b, dst, M, kHidden))) return rc;
    }
    if (nl == 0 && (rc = run_copy(e, s, out, x0, (size_t)M * kHidden))) return rc;
    if (hidden_states && hidden_states[nl] && (rc = run_copy(e, s, hidden_states[nl], out, (size_t)M * kHidden))) return rc;
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
    int rc;
    static const char* const kConvNames[7] = {"feature_encoder.conv_layers.0 (GroupNorm + GELU)", "feature_encoder.conv_layers.1",
                                              "feature_encoder.conv_layers.2", "feature_encoder.conv_layers.3",
                                              "feature_encoder.conv_layers.4", "feature_encoder.conv_layers.5",
                                              "feature_encoder.conv_layers.6"};
    // ---- feature encoder: conv0 writes planes, conv1-5 planes -> planes, conv6 planes -> fp32 (LayerNorm input)
    _Float16 *ihi, *ilo, *ohi, *olo;
    planes(bf.bufA, (size_t)B * p.Tc[0] * kConvDim, ihi, ilo);
    if ((rc = run_conv0(e, s, p, wav, bf, nullptr, ihi, ilo, c.slot(kConvNames[0])))) return rc;
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
        if ((rc = run_gemm_split(e, c, s, a, e->conv_s[i]))) return rc;
        std::swap(cin, cout);
    }
    float* feats = cin;  // [M,512] fp32
    if (e->tap_conv && (rc = run_copy(e, s, e->tap_conv, feats, (size_t)M * kConvDim))) return rc;

    // ---- feature projection: LayerNorm(512) -> planes (in the idle conv buffer) -> Linear(512,768) -> x1 fp32
    planes(cout, (size_t)M * kConvDim, ohi, olo);
    if ((rc = run_ln(e, s, feats, sw.proj_norm.w, sw.proj_norm.b, nullptr, M, kConvDim, ohi, olo))) return rc;
    GemmSplitArgs a = split_args(M, kHidden, kConvDim, kEpiNone);
    a.Ahi = ohi; a.Alo = olo; a.bias = sw.proj.b; a.C = bf.x1;
    if ((rc = run_gemm_split(e, c, s, a, e->proj_s))) return rc;
    if (e->tap_proj && (rc = run_copy(e, s, e->tap_proj, bf.x1, (size_t)M * kHidden))) return rc;

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
    if ((rc = run_gemm_split(e, c, s, a, e->posg_s, K_POSCONV_SPLIT, 2.0 * M * (double)kHidden * kPosCg * kPosK, 8.0 * M * kHidden)))
        return rc;
    if (e->tap_prenet && (rc = run_copy(e, s, e->tap_prenet, bf.x0, (size_t)M * kHidden))) return rc;
    return LOCO_OK;
}

int encoder_f16x3(loco_encoder* e, Call& c, const Plan& p, float* out, float* const* hidden_states, const Bufs& bf, hipStream_t s) {
    const int B = p.B;
    const int T = (int)p.T;
    const long M = p.M;
    const int F = e->cfg.ffn;
    const size_t MH = (size_t)M * kHidden;
    int rc;
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
    if ((rc = run_ln(e, s, x0, e->stem.layer_norm.w, e->stem.layer_norm.b, x0f, M, kHidden, x0hi, x0lo))) return rc;
    for (int l = 0; l < nl; ++l) {
        if (hidden_states && hidden_states[l] && (rc = run_copy(e, s, hidden_states[l], x0, MH))) return rc;
        const LayerW& lw = e->layers[l];
        // fused q|k|v projection -> q, k and v as fp16 hi/lo planes [M,768] (the layout attention_f16x3 reads; it transposes V itself)
        GemmSplitArgs a = split_args(M, kQkv, kHidden, kEpiQkvScatter);
        a.Ahi = x0hi; a.Alo = x0lo; a.bias = lw.bqkv;
        a.Chi = qshi; a.Clo = qslo; a.ldc = kHidden; a.qkv_stride = (long)2 * M * kHidden; a.T = T;
        a.range_slot = c.slot("attention q|k|v projections", l);
        if ((rc = run_gemm_split(e, c, s, a, lw.sqkv))) return rc;
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
        // the table the launch just formed in bf.qp holds every column a valid key reads (include/loco_asr.h)
        if ((rc = run_attention_probs(e, s, nullptr, qshi, qslo, kshi, kslo, bf.qp, bf.frames_or_null, l, B, T))) return rc;
        dbg_planes(e, s, "attention context planes %s", l, chi, clo, MH, kHidden);
        // out_proj + residual, LayerNorm
        a = split_args(M, kHidden, kHidden, kEpiResidual);
        a.Ahi = chi; a.Alo = clo; a.bias = lw.out_proj.b;
        a.Rhi = x0hi; a.Rlo = x0lo; a.ldr = kHidden; a.C = tmp;
        if ((rc = run_gemm_split(e, c, s, a, lw.so))) return rc;
        dbg_check(e, s, "out_proj + residual (fp32)", l, tmp, MH, false, kHidden);
        if ((rc = run_ln(e, s, tmp, lw.layer_norm.w, lw.layer_norm.b, nullptr, M, kHidden, x1hi, x1lo))) return rc;
        dbg_planes(e, s, "layer_norm planes %s", l, x1hi, x1lo, MH, kHidden);
        // FFN + residual + final LayerNorm
        a = split_args(M, F, kHidden, kEpiGelu);
        a.Ahi = x1hi; a.Alo = x1lo; a.bias = lw.ffn_in.b;
        a.Chi = fhi; a.Clo = flo; a.range_slot = c.slot("feed_forward intermediate (GELU)", l);
        if ((rc = run_gemm_split(e, c, s, a, lw.s1))) return rc;
        dbg_planes(e, s, "feed_forward intermediate planes %s", l, fhi, flo, (size_t)M * F, F);
        a = split_args(M, kHidden, F, kEpiResidual);
        a.Ahi = fhi; a.Alo = flo; a.bias = lw.ffn_out.b;
        a.Rhi = x1hi; a.Rlo = x1lo; a.ldr = kHidden; a.C = tmp;
        if ((rc = run_gemm_split(e, c, s, a, lw.s2))) return rc;
        dbg_check(e, s, "feed_forward output + residual (fp32)", l, tmp, MH, false, kHidden);
        const bool last = l == nl - 1;
        if ((rc = run_ln(e, s, tmp, lw.final_layer_norm.w, lw.final_layer_norm.b, last ? out : (hidden_states ? x0 : nullptr), M, kHidden,
                         last ? nullptr : x0hi, last ? nullptr : x0lo,
                         last && c.range_dev ? c.range_dev + (size_t)kRangeShards * kFiniteStage : nullptr)))
            return rc;
    }
    if (nl == 0 && (rc = run_copy(e, s, out, x0, MH))) return rc;
    if (hidden_states && hidden_states[nl] && (rc = run_copy(e, s, hidden_states[nl], out, MH))) return rc;
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

}  // namespace

extern "C" {

int loco_abi_version(void) { return LOCO_ABI_VERSION; }

const char* loco_last_error(void) { return g_err.c_str(); }

void loco_default_config(loco_config* c) {
    if (!c) return;
    c->struct_size = (int32_t)sizeof(loco_config);
    c->hidden = kHidden;
    c->heads = kHeads;
    c->ffn = kFfn;
    c->layers = 12;
    c->conv_dim = kConvDim;
    c->pos_conv_kernel = kPosK;
    c->pos_conv_groups = kPosGroups;
    c->rel_max = kRelMax;
    c->ln_eps = 1e-5f;
}

loco_encoder* loco_create(const loco_config* cfg) {
    loco_config c;
    loco_default_config(&c);
    if (cfg) {
        if (cfg->struct_size != (int32_t)sizeof(loco_config)) {
            fail(LOCO_E_INVALID, "loco_config.struct_size %d != %zu", cfg->struct_size, sizeof(loco_config));
            return nullptr;
        }
        c = *cfg;
    }
    if (c.hidden != kHidden || c.heads != kHeads || c.ffn != kFfn || c.conv_dim != kConvDim ||
        c.pos_conv_kernel != kPosK || c.pos_conv_groups != kPosGroups || c.rel_max != kRelMax || c.layers < 0 ||
        c.layers > 64) {
        fail(LOCO_E_INVALID, "unsupported configuration: kernels are specialised for SpeechT5-base (768/12/3072/512/128/16/160)");
        return nullptr;
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        fail(LOCO_E_HIP, "hipGetDevice failed: no usable HIP device");
        return nullptr;
    }
    loco_encoder* e = new loco_encoder();
    e->cfg = c;
    e->device = dev;
    if (hipHostMalloc(reinterpret_cast<void**>(&e->own), sizeof(StatusBlock), hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&e->absmax_dev, sizeof(float)) != hipSuccess) {
        fail(LOCO_E_HIP, "loco_create: could not allocate the range-status block");
        if (e->own) (void)hipHostFree(e->own);
        delete e;
        return nullptr;
    }
    memset(e->own, 0, sizeof(StatusBlock));
    e->own->magic = kStatusMagic;
    if (const char* dbg = getenv("LOCO_DEBUG_NONFINITE")) {
        e->debug_nonfinite = dbg[0] == '1' && hipMalloc(&e->debug_counter, 2 * sizeof(unsigned long long)) == hipSuccess;
    }
    e->layers.resize(c.layers);
    build_expected(e);
    for (int i = 0; i < K_COUNT; ++i) {
        memset(&e->stats[i], 0, sizeof(loco_kernel_stat));
        snprintf(e->stats[i].name, sizeof e->stats[i].name, "%s", kKernelNames[i]);
    }
    return e;
}

void loco_destroy(loco_encoder* e) {
    if (!e) return;
    for (auto& kv : e->raw) (void)hipFree(kv.second);
    for (int i = 1; i < 7; ++i) (void)hipFree(e->conv_w[i]);
    (void)hipFree(e->pos_w);
    auto free_split = [](SplitW& w) {
        (void)hipFree(w.hi);
        (void)hipFree(w.lo);
    };
    for (int i = 1; i < 7; ++i) free_split(e->conv_s[i]);
    free_split(e->proj_s);
    free_split(e->pe_s);
    free_split(e->posg_s);
    for (auto& l : e->layers) {
        (void)hipFree(l.wqkv);
        (void)hipFree(l.bqkv);
        free_split(l.sqkv);
        free_split(l.so);
        free_split(l.s1);
        free_split(l.s2);
    }
    for (auto& l : e->dec.L) {
        (void)hipFree(l.wqkv);
        (void)hipFree(l.bqkv);
        (void)hipFree(l.wcq);
        (void)hipFree(l.bcq);
    }
    (void)hipFree(e->dec.wckv);
    (void)hipFree(e->dec.bckv);
    (void)hipFree(e->dec.pos_tab);
    if (e->dec.host_state) (void)hipHostFree(e->dec.host_state);
    (void)hipFree(e->absmax_dev);
    (void)hipFree(e->debug_counter);
    if (e->own) (void)hipHostFree(e->own);
    (void)hipFree(e->sin_tab.load());
    for (float* t : e->retired) (void)hipFree(t);
    (void)hipFree(e->text_embed);
    (void)hipFree(e->text_alpha);
    (void)hipFree(e->text_pe);
    if (e->side) {
        (void)hipStreamDestroy(e->side);
        (void)hipEventDestroy(e->ev_fork);
        (void)hipEventDestroy(e->ev_join);
    }
    for (auto& r : e->recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    delete e;
}

int loco_set_weight(loco_encoder* e, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!e || !key || !data || !shape || ndim < 1 || ndim > 4) return fail(LOCO_E_INVALID, "loco_set_weight: null/invalid argument");
    const std::string k = canonical_key(key);
    std::vector<int64_t> shp(shape, shape + ndim);
    int64_t n = 1;
    for (auto s : shp) n *= s;
    if (k == "prenet.pos_sinusoidal_embed.weights") {
        if (ndim != 2 || shp[1] != kHidden || shp[0] < 3) return fail(LOCO_E_INVALID, "%s: expected [rows,768]", key);
        float* d = nullptr;
        HIP_TRY(hipMalloc(&d, (size_t)n * sizeof(float)));
        HIP_TRY(hipMemcpy(d, data, (size_t)n * sizeof(float), hipMemcpyDefault));
        HIP_TRY(hipDeviceSynchronize());
        {   // a weight load: the caller guarantees no forward is in flight (as for every loco_set_weight)
            std::lock_guard<std::mutex> lock(e->sin_mu);
            (void)hipFree(e->sin_tab.load(std::memory_order_relaxed));
            e->sin_rows.store(0, std::memory_order_release);
            e->sin_tab.store(d, std::memory_order_release);
            e->sin_rows.store((int)shp[0], std::memory_order_release);
        }
        e->sin_user = true;
        return LOCO_OK;
    }
    if (k.rfind("text_prenet.", 0) == 0) {
        // SpeechT5TextEncoderPrenet.state_dict(): embed_tokens.weight [V,768], encode_positions.alpha [] (pass as [1]);
        // encode_positions.pe [1,rows,768] or [rows,768] is a non-persistent buffer in current HF, a key in 4.30's pickles
        float** slot = nullptr;
        if (k == "text_prenet.embed_tokens.weight") {
            if (ndim != 2 || shp[1] != kHidden || shp[0] < 1) return fail(LOCO_E_INVALID, "%s: expected [vocab,768]", key);
            slot = &e->text_embed;
            e->text_vocab = (int)shp[0];
        } else if (k == "text_prenet.encode_positions.alpha") {
            if (n != 1) return fail(LOCO_E_INVALID, "%s: expected one element", key);
            slot = &e->text_alpha;
        } else if (k == "text_prenet.encode_positions.pe") {
            if (!((ndim == 2 && shp[1] == kHidden) || (ndim == 3 && shp[0] == 1 && shp[2] == kHidden)))
                return fail(LOCO_E_INVALID, "%s: expected [rows,768] or [1,rows,768]", key);
            slot = &e->text_pe;
            e->text_pe_rows = (int)(n / kHidden);
        } else {
            return fail(LOCO_E_INVALID, "unexpected key in state_dict: %s", key);
        }
        float* d = nullptr;
        HIP_TRY(hipMalloc(&d, (size_t)n * sizeof(float)));
        HIP_TRY(hipMemcpy(d, data, (size_t)n * sizeof(float), hipMemcpyDefault));
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(*slot);
        *slot = d;
        return LOCO_OK;
    }
    if (k == "decoder.prenet.embed_positions.weights") {  // HF's non-persistent buffer: given, it replaces the generated table
        if (ndim != 2 || shp[1] != kHidden || shp[0] < kDecMaxPositions + 2) return fail(LOCO_E_INVALID, "%s: expected [>= 452,768]", key);
        float* d = nullptr;
        HIP_TRY(hipMalloc(&d, (size_t)n * sizeof(float)));
        HIP_TRY(hipMemcpy(d, data, (size_t)n * sizeof(float), hipMemcpyDefault));
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(e->dec.pos_tab);
        e->dec.pos_tab = d;
        e->dec.pos_rows = (int)shp[0];
        e->dec.pos_user = true;
        return LOCO_OK;
    }
    std::vector<int64_t> dec_shape;
    const bool dec_key = decoder_key_shape(k, shp, dec_shape);
    auto it = e->expected.find(k);
    if (!dec_key && it == e->expected.end()) return fail(LOCO_E_INVALID, "unexpected key in state_dict: %s", key);
    if ((dec_key ? dec_shape : it->second) != shp) {
        std::string got, want;
        for (auto s : shp) got += std::to_string(s) + ",";
        for (auto s : (dec_key ? dec_shape : it->second)) want += std::to_string(s) + ",";
        return fail(LOCO_E_INVALID, "size mismatch for %s: got [%s] expected [%s]", key, got.c_str(), want.c_str());
    }
    float*& d = e->raw[k];
    // [vocab,768]: the only tensors whose size is the checkpoint's own -- a re-load with another vocabulary gets a new buffer
    if (d && (k == kDecEmbedKey || k == kDecHeadKey) && e->dec_shapes.count(k) && e->dec_shapes[k] != shp) {
        (void)hipFree(d);
        d = nullptr;
    }
    if (dec_key) e->dec_shapes[k] = shp;
    if (!d) HIP_TRY(hipMalloc(&d, (size_t)n * sizeof(float)));
    HIP_TRY(hipMemcpy(d, data, (size_t)n * sizeof(float), hipMemcpyDefault));
    HIP_TRY(hipStreamSynchronize(nullptr));  // device-to-device copies may return early; the caller may free `data` now
    e->finalized = false;
    return LOCO_OK;
}

int loco_missing_weights(const loco_encoder* e, char* buf, size_t buflen) {
    if (!e) return fail(LOCO_E_INVALID, "null encoder");
    int missing = 0;
    std::string names;
    bool any_speech = false;
    for (auto& kv : e->raw) any_speech = any_speech || kv.first.rfind("prenet.", 0) == 0;
    const bool text_only = e->text_embed && !any_speech;  // a text-encoder handle: the speech prenet is not required
    for (auto& kv : e->expected) {
        if (optional_key(kv.first) || e->raw.count(kv.first)) continue;
        if (text_only && kv.first.rfind("prenet.", 0) == 0) continue;
        ++missing;
        if (!names.empty()) names += ",";
        names += kv.first;
    }
    if (e->text_embed && !e->text_alpha) {
        ++missing;
        names += (names.empty() ? "" : ",") + std::string("text_prenet.encode_positions.alpha");
    }
    missing += decoder_missing(e, &names);
    if (buf && buflen) snprintf(buf, buflen, "%s", names.c_str());
    return missing;
}

namespace {
// Decoder weights as the kernels read them: q|k|v of the self-attention fused ([2304,768], the 1/8 query scaling folded in -- exact, a
// power of two), the cross-attention q scaled alike, the cross-attention k|v of ALL layers stacked into one [layers * 1536, 768]
// operand (projected once per utterance by one big-M GEMM).  The tied embedding / lm_head pair: either one serves for both.
int finalize_decoder(loco_encoder* e, hipStream_t s) {
    DecoderW& d = e->dec;
    bool any = false;
    const int layers = decoder_layers_loaded(e, &any);
    d.ready = false;
    if (!any) return LOCO_OK;
    const size_t hh = (size_t)kHidden * kHidden;
    if ((int)d.L.size() != layers) {
        for (auto& l : d.L) {
            (void)hipFree(l.wqkv), (void)hipFree(l.bqkv), (void)hipFree(l.wcq), (void)hipFree(l.bcq);
        }
        d.L.assign(layers, DecLayerW());
        (void)hipFree(d.wckv), (void)hipFree(d.bckv);
        d.wckv = d.bckv = nullptr;
    }
    d.layers = layers;
    if (!d.wckv) HIP_TRY(hipMalloc(&d.wckv, (size_t)layers * 2 * hh * sizeof(float)));
    if (!d.bckv) HIP_TRY(hipMalloc(&d.bckv, (size_t)layers * 2 * kHidden * sizeof(float)));
    for (int l = 0; l < layers; ++l) {
        DecLayerW& lw = d.L[l];
        const std::string b = "decoder.wrapped_decoder.layers." + std::to_string(l) + ".", sa = b + "self_attn.", ca = b + "encoder_attn.";
        if (!lw.wqkv) HIP_TRY(hipMalloc(&lw.wqkv, 3 * hh * sizeof(float)));
        if (!lw.bqkv) HIP_TRY(hipMalloc(&lw.bqkv, 3 * kHidden * sizeof(float)));
        if (!lw.wcq) HIP_TRY(hipMalloc(&lw.wcq, hh * sizeof(float)));
        if (!lw.bcq) HIP_TRY(hipMalloc(&lw.bcq, kHidden * sizeof(float)));
        HIP_TRY(launch_scale_copy(W(e, sa + "q_proj.weight"), lw.wqkv, hh, 0.125f, s));
        HIP_TRY(launch_scale_copy(W(e, sa + "k_proj.weight"), lw.wqkv + hh, hh, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, sa + "v_proj.weight"), lw.wqkv + 2 * hh, hh, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, sa + "q_proj.bias"), lw.bqkv, kHidden, 0.125f, s));
        HIP_TRY(launch_scale_copy(W(e, sa + "k_proj.bias"), lw.bqkv + kHidden, kHidden, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, sa + "v_proj.bias"), lw.bqkv + 2 * kHidden, kHidden, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, ca + "q_proj.weight"), lw.wcq, hh, 0.125f, s));
        HIP_TRY(launch_scale_copy(W(e, ca + "q_proj.bias"), lw.bcq, kHidden, 0.125f, s));
        HIP_TRY(launch_scale_copy(W(e, ca + "k_proj.weight"), d.wckv + (size_t)l * 2 * hh, hh, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, ca + "v_proj.weight"), d.wckv + (size_t)l * 2 * hh + hh, hh, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, ca + "k_proj.bias"), d.bckv + (size_t)l * 2 * kHidden, kHidden, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, ca + "v_proj.bias"), d.bckv + (size_t)l * 2 * kHidden + kHidden, kHidden, 1.0f, s));
        lw.self_out = weight_bias(e, sa + "out_proj.");
        lw.self_ln = weight_bias(e, b + "self_attn_layer_norm.");
        lw.cross_out = weight_bias(e, ca + "out_proj.");
        lw.cross_ln = weight_bias(e, b + "encoder_attn_layer_norm.");
        lw.ffn_in = weight_bias(e, b + "feed_forward.intermediate_dense.");
        lw.ffn_out = weight_bias(e, b + "feed_forward.output_dense.");
        lw.final_ln = weight_bias(e, b + "final_layer_norm.");
    }
    const bool has_embed = e->raw.count(kDecEmbedKey) != 0, has_head = e->raw.count(kDecHeadKey) != 0;
    d.embed = W(e, has_embed ? kDecEmbedKey : kDecHeadKey);
    d.lm_head = W(e, has_head ? kDecHeadKey : kDecEmbedKey);
    const std::vector<int64_t>&se = e->dec_shapes.at(has_embed ? kDecEmbedKey : kDecHeadKey), &sh = e->dec_shapes.at(has_head ? kDecHeadKey : kDecEmbedKey);
    if (se[0] != sh[0]) return fail(LOCO_E_INVALID, "decoder: embed_tokens has %lld rows, lm_head %lld", (long long)se[0], (long long)sh[0]);
    d.vocab = (int)se[0];
    if (!d.pos_tab) {  // C callers without HF's buffer: the library's own generator (the same torch expression, fp32 step by step)
        d.pos_rows = kDecMaxPositions + 2;
        HIP_TRY(hipMalloc(&d.pos_tab, (size_t)d.pos_rows * kHidden * sizeof(float)));
        HIP_TRY(launch_sinusoid_table(d.pos_tab, d.pos_rows, s));
    }
    if (!d.host_state) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&d.host_state), 4 * sizeof(int32_t), hipHostMallocDefault));
    d.ready = true;
    return LOCO_OK;
}
}  // namespace

int loco_finalize_weights(loco_encoder* e, void* stream) {
    if (!e) return fail(LOCO_E_INVALID, "null encoder");
    hipStream_t s = (hipStream_t)stream;
    char names[256];
    const int miss = loco_missing_weights(e, names, sizeof names);
    if (miss) return fail(LOCO_E_STATE, "%d weights missing: %s", miss, names);
    const std::string p = "prenet.", w = "wrapped_encoder.";
    const bool speech = e->raw.count(p + "feature_encoder.conv_layers.0.conv.weight") != 0;
    e->speech_ready = false;
    if (e->text_embed && !e->text_pe) {  // C callers without HF's table: 1024 rows from the library's own generator
        HIP_TRY(hipMalloc(&e->text_pe, (size_t)1024 * kHidden * sizeof(float)));
        HIP_TRY(launch_text_pe_table(e->text_pe, 1024, s));
        e->text_pe_rows = 1024;
    }
    // conv layers 1..6: [512,512,k] -> [512, k*512]
    for (int i = 1; speech && i < 7; ++i) {
        const size_t n = (size_t)kConvDim * kConvDim * kConvK[i];
        if (!e->conv_w[i]) HIP_TRY(hipMalloc(&e->conv_w[i], n * sizeof(float)));
        HIP_TRY(launch_relayout_conv_weight(W(e, p + "feature_encoder.conv_layers." + std::to_string(i) + ".conv.weight"),
                                            e->conv_w[i], kConvDim, kConvDim, kConvK[i], s));
    }
    StemW& sw = e->stem;
    if (speech) {
        sw.conv0_norm = weight_bias(e, p + "feature_encoder.conv_layers.0.layer_norm.");
        sw.proj_norm = weight_bias(e, p + "feature_projection.layer_norm.");
        sw.proj = weight_bias(e, p + "feature_projection.projection.");
        sw.pos_b = W(e, p + "pos_conv_embed.conv.bias");
        e->conv_w[0] = e->raw.at(p + "feature_encoder.conv_layers.0.conv.weight");
        // positional conv: fold weight-norm, lay out [group][tap][o][i]
        if (!e->pos_w) HIP_TRY(hipMalloc(&e->pos_w, (size_t)kHidden * kPosCg * kPosK * sizeof(float)));
        HIP_TRY(launch_fold_pos_conv(W(e, p + "pos_conv_embed.conv.parametrizations.weight.original0"),
                                     W(e, p + "pos_conv_embed.conv.parametrizations.weight.original1"), e->pos_w, s));
    }
    // fused QKV with the 1/8 query scaling folded in: (x Wq^T + bq)/8 == x (Wq/8)^T + bq/8 exactly (power of two)
    sw.layer_norm = weight_bias(e, w + "layer_norm.");
    sw.pe_k = W(e, w + "embed_positions.pe_k.weight");
    const size_t hh = (size_t)kHidden * kHidden;
    for (int l = 0; l < e->cfg.layers; ++l) {
        LayerW& lw = e->layers[l];
        const std::string b = w + "layers." + std::to_string(l) + ".", a = b + "attention.";
        if (!lw.wqkv) HIP_TRY(hipMalloc(&lw.wqkv, 3 * hh * sizeof(float)));
        if (!lw.bqkv) HIP_TRY(hipMalloc(&lw.bqkv, 3 * kHidden * sizeof(float)));
        HIP_TRY(launch_scale_copy(W(e, a + "q_proj.weight"), lw.wqkv, hh, 0.125f, s));
        HIP_TRY(launch_scale_copy(W(e, a + "k_proj.weight"), lw.wqkv + hh, hh, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, a + "v_proj.weight"), lw.wqkv + 2 * hh, hh, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, a + "q_proj.bias"), lw.bqkv, kHidden, 0.125f, s));
        HIP_TRY(launch_scale_copy(W(e, a + "k_proj.bias"), lw.bqkv + kHidden, kHidden, 1.0f, s));
        HIP_TRY(launch_scale_copy(W(e, a + "v_proj.bias"), lw.bqkv + 2 * kHidden, kHidden, 1.0f, s));
        lw.out_proj = weight_bias(e, a + "out_proj.");
        lw.layer_norm = weight_bias(e, b + "layer_norm.");
        lw.ffn_in = weight_bias(e, b + "feed_forward.intermediate_dense.");
        lw.ffn_out = weight_bias(e, b + "feed_forward.output_dense.");
        lw.final_layer_norm = weight_bias(e, b + "final_layer_norm.");
    }
    // fp16 hi/lo planes of every GEMM weight for precision mode f16x3 (378 MB; built unconditionally so that the
    // mode can be switched per forward)
    int rc = LOCO_OK;
    for (int i = 1; speech && i < 7 && !rc; ++i) {  // conv planes in the channel-block-major k order the GEMM walks (GemmSplitArgs::ktaps)
        const size_t n = (size_t)kConvDim * kConvDim * kConvK[i];
        float* tmpw = nullptr;
        HIP_TRY(hipMalloc(&tmpw, n * sizeof(float)));
        const hipError_t he = launch_permute_conv_k(e->conv_w[i], tmpw, kConvDim, kConvK[i], kConvDim, s);
        if (he == hipSuccess) rc = make_split(e, e->conv_s[i], tmpw, n, s);
        HIP_TRY(hipStreamSynchronize(s));
        (void)hipFree(tmpw);
        if (he != hipSuccess) return fail(LOCO_E_HIP, "permute_conv_k: %s", hipGetErrorString(he));
    }
    if (speech && !rc) rc = make_split(e, e->proj_s, sw.proj.w, (size_t)kHidden * kConvDim, s);
    if (!rc) rc = make_split(e, e->pe_s, sw.pe_k, (size_t)kRelN * kHeadDim, s);
    if (speech && !rc) {  // positional conv weight re-laid [g][o][tap*48+i] for the conv-as-GEMM form, then split
        float* tmpw = nullptr;
        const size_t n = (size_t)kHidden * kPosCg * kPosK;
        HIP_TRY(hipMalloc(&tmpw, n * sizeof(float)));
        hipError_t he = launch_pos_w_for_gemm(e->pos_w, tmpw, s);
        if (he == hipSuccess) rc = make_split(e, e->posg_s, tmpw, n, s);
        HIP_TRY(hipStreamSynchronize(s));
        (void)hipFree(tmpw);
        if (he != hipSuccess) return fail(LOCO_E_HIP, "pos_w_for_gemm: %s", hipGetErrorString(he));
    }
    for (int l = 0; l < e->cfg.layers && !rc; ++l) {
        LayerW& lw = e->layers[l];
        rc = make_split(e, lw.sqkv, lw.wqkv, 3 * hh, s);
        if (!rc) rc = make_split(e, lw.so, lw.out_proj.w, hh, s);
        if (!rc) rc = make_split(e, lw.s1, lw.ffn_in.w, (size_t)e->cfg.ffn * kHidden, s);
        if (!rc) rc = make_split(e, lw.s2, lw.ffn_out.w, (size_t)e->cfg.ffn * kHidden, s);
    }
    if (rc) return rc;
    if (speech) {
        const float* unused_tab = nullptr;
        rc = ensure_sin_rows(e, 4002, s, &unused_tab);
        if (rc) return rc;
    }
    // weight-determined activation ranges of precision mode f16x3 (static_range_check above)
    // (conv0's GroupNorm + GELU output is not among them: its bound sqrt(frames per clip) * max|gamma| + max|beta| says nothing
    // useful for 10-minute clips -- 1385 * max|gamma| -- so conv0_apply_kernel folds max|x| of what it writes like the GEMMs do)
    e->range_static.clear();
    if (speech) rc = static_range_check(e, p + "feature_projection.layer_norm.", kConvDim, s);
    if (!rc) rc = static_range_check(e, w + "layer_norm.", kHidden, s);
    for (int l = 0; l < e->cfg.layers && !rc; ++l) {
        const std::string b = w + "layers." + std::to_string(l) + ".";
        rc = static_range_check(e, b + "layer_norm.", kHidden, s);
        if (!rc && l + 1 < e->cfg.layers) rc = static_range_check(e, b + "final_layer_norm.", kHidden, s);  // the last one is written in fp32
    }
    if (rc) return rc;
    rc = finalize_decoder(e, s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    e->speech_ready = speech;
    e->finalized = true;
    return LOCO_OK;
}

int64_t loco_output_frames(int64_t n) {
    for (int i = 0; i < 7; ++i) {
        const int64_t d = n - kConvK[i];
        n = (d >= 0 ? d / kConvS[i] : -((-d + kConvS[i] - 1) / kConvS[i])) + 1;
    }
    return n;
}

namespace {
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
}  // namespace

size_t loco_workspace_bytes(const loco_encoder* e, int32_t B, int64_t L) {
    Plan p, p0, p1;
    if (!e || !make_plan(e, B, L, p)) return 0;
    if (split_batch(e, B, L, p0, p1)) return kStatusDevBytes + std::max(p.total, p0.total + p1.total);
    return kStatusDevBytes + p.total;
}

int loco_set_streams(loco_encoder* e, int n) {
    if (!e || (n != 1 && n != 2)) return fail(LOCO_E_INVALID, "loco_set_streams: n must be 1 or 2");
    e->streams = n;
    return LOCO_OK;
}

const char* loco_precision_name(int mode) {
    static const char* const kNames[] = {"f32", "f16x3", "f16x2"};
    return (mode >= 0 && mode < 3) ? kNames[mode] : nullptr;
}

int loco_set_precision(loco_encoder* e, int mode) {
    if (!e || !loco_precision_name(mode)) return fail(LOCO_E_INVALID, "loco_set_precision: mode must be 0 (f32), 1 (f16x3) or 2 (f16x2)");
    e->precision = mode;
    return LOCO_OK;
}

int loco_get_precision(const loco_encoder* e) { return e ? e->precision : LOCO_E_INVALID; }

int loco_set_taps(loco_encoder* e, float* conv_stack, float* feature_projection, float* prenet) {
    if (!e) return fail(LOCO_E_INVALID, "null encoder");
    e->tap_conv = conv_stack;
    e->tap_proj = feature_projection;
    e->tap_prenet = prenet;
    return LOCO_OK;
}

int loco_set_attention_outputs(loco_encoder* e, float* const* probs, int32_t n) {
    if (!e) return fail(LOCO_E_INVALID, "null encoder");
    if (!probs) {
        e->attn_probs.clear();
        return LOCO_OK;
    }
    if (n != e->cfg.layers)
        return fail(LOCO_E_INVALID, "loco_set_attention_outputs: %d buffers for %d layers", n, e->cfg.layers);
    for (int i = 0; i < n; ++i)
        if (!probs[i]) return fail(LOCO_E_INVALID, "loco_set_attention_outputs: buffer %d is null", i);
    e->attn_probs.assign(probs, probs + n);
    return LOCO_OK;
}

namespace {
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

const StatusBlock* as_status(const void* status) {
    const StatusBlock* st = reinterpret_cast<const StatusBlock*>(status);
    return (st && st->magic == kStatusMagic) ? st : nullptr;
}

float stage_amax(const StatusBlock* st, int i) {
    float amax = 0.f;
    for (int k = 0; k < kRangeShards; ++k) amax = fmaxf(amax, st->words[(size_t)i * kRangeShards + k]);
    return amax;
}

int status_check(const StatusBlock* st, char* buf, size_t buflen) {
    if (buf && buflen) buf[0] = 0;
    if (st->precision == 0) return LOCO_OK;  // the exact-fp32 mode stores no fp16 planes
    if (st->msg[0]) {
        if (buf && buflen) snprintf(buf, buflen, "%s", st->msg);
        return fail(LOCO_E_RANGE, "%s; use the exact-fp32 kernels for this model (loco_set_precision(enc, 0) / loco_forward_checked)", st->msg);
    }
    for (int i = 0; i < st->used; ++i) {
        const float amax = stage_amax(st, i);
        const bool over = !(amax < kRangeHi), under = amax < kRangeLo;
        if (!over && !under) continue;
        char where[160];
        if (st->layer[i] >= 0) snprintf(where, sizeof where, "wrapped_encoder.layers.%d %s", st->layer[i], st->names[i]);
        else snprintf(where, sizeof where, "%s", st->names[i]);
        char msg[400];
        snprintf(msg, sizeof msg,
                 "activation range: max|x| = %.6g of '%s' is %s the range precision mode f16x3 represents to fp32 class "
                 "(%g <= max|x| < %g); use the exact-fp32 kernels for this input (loco_set_precision(enc, 0) / loco_forward_checked)",
                 (double)amax, where, over ? "above" : "below", (double)kRangeLo, (double)kRangeHi);
        if (buf && buflen) snprintf(buf, buflen, "%s", msg);
        return fail(LOCO_E_RANGE, "%s", msg);
    }
    // the finite check of the last LayerNorm: the range words above are maxima taken with fmaxf, which a NaN never enters -- an
    // inf / NaN born inside a stage (not by leaving the range of a tracked plane tensor) is caught where everything ends up
    if (st->used > 0 && stage_amax(st, kFiniteStage) > 0.f) {
        const char* msg = "activation range: last_hidden_state holds non-finite values (inf / NaN) although every tracked plane tensor "
                          "stayed inside the range precision mode f16x3 represents; use the exact-fp32 kernels for this input "
                          "(loco_set_precision(enc, 0) / loco_forward_checked)";
        if (buf && buflen) snprintf(buf, buflen, "%s", msg);
        return fail(LOCO_E_RANGE, "%s", msg);
    }
    return LOCO_OK;
}

int status_range(const StatusBlock* st, int32_t stage, float* amax, int32_t* layer, char* name, size_t namelen) {
    if (stage < 0 || stage >= st->used) return st->used;  // not an error: lets a caller enumerate 0 .. n-1
    if (amax) *amax = stage_amax(st, stage);
    if (layer) *layer = st->layer[stage];
    if (name && namelen) snprintf(name, namelen, "%s", st->names[stage]);
    return st->used;
}
}  // namespace

int loco_forward(loco_encoder* e, const float* wav, const int32_t* mask, int32_t B, int64_t L, float* out,
                 int32_t* out_frames, float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e) return fail(LOCO_E_INVALID, "loco_forward: null argument");
    return forward_impl(e, e->precision, e->own, wav, mask, B, L, out, out_frames, hidden_states, workspace, workspace_bytes, stream);
}

// ---- forwards in flight: one status block per forward (include/loco_asr.h) ---------------------------------------------------
size_t loco_status_bytes(void) { return sizeof(StatusBlock); }

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

int loco_status_check(const void* status, char* buf, size_t buflen) {
    const StatusBlock* st = as_status(status);
    if (!st) return fail(LOCO_E_INVALID, "loco_status_check: not a status block filled by loco_forward_async");
    return status_check(st, buf, buflen);
}

int loco_status_range(const void* status, int32_t stage, float* amax, int32_t* layer, char* name, size_t namelen) {
    const StatusBlock* st = as_status(status);
    if (!st) return fail(LOCO_E_INVALID, "loco_status_range: not a status block filled by loco_forward_async");
    return status_range(st, stage, amax, layer, name, namelen);
}

// ---- range status of the last forward enqueued through loco_forward / loco_forward_text (include/loco_asr.h) ------------------
int loco_forward_status(loco_encoder* e, char* buf, size_t buflen) {
    if (!e) return fail(LOCO_E_INVALID, "null encoder");
    return status_check(e->own, buf, buflen);
}

int loco_forward_range(const loco_encoder* e, int32_t stage, float* amax, int32_t* layer, char* name, size_t namelen) {
    if (!e) return fail(LOCO_E_INVALID, "null encoder");
    return status_range(e->own, stage, amax, layer, name, namelen);
}

int loco_set_range_policy(loco_encoder* e, int policy) {
    if (!e || (policy != 0 && policy != 1)) return fail(LOCO_E_INVALID, "loco_set_range_policy: policy must be 0 (report) or 1 (re-run in fp32)");
    e->range_policy = policy;
    return LOCO_OK;
}

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

namespace {
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

// ---- profiling -----------------------------------------------------------------------------------------
int loco_set_profiling(loco_encoder* e, int on) {
    if (!e) return fail(LOCO_E_INVALID, "null encoder");
    e->profiling = on != 0;
    return LOCO_OK;
}

int loco_set_profiling_filter(loco_encoder* e, const char* bucket) {
    if (!e) return fail(LOCO_E_INVALID, "null encoder");
    if (!bucket || !*bucket) {
        e->profile_only = -1;
        return LOCO_OK;
    }
    for (int i = 0; i < K_COUNT; ++i)
        if (!strcmp(bucket, kKernelNames[i])) {
            e->profile_only = i;
            return LOCO_OK;
        }
    return fail(LOCO_E_INVALID, "loco_set_profiling_filter: no kernel bucket named '%s'", bucket);
}

static int drain_records(loco_encoder* e) {
    for (size_t i = 0; i < e->recs_used; ++i) {
        ProfRec& r = e->recs[i];
        HIP_TRY(hipEventSynchronize(r.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        loco_kernel_stat& st = e->stats[r.kid];
        st.launches += 1;
        st.ms += ms;
        st.flops += r.flops;
        st.bytes += r.bytes;
    }
    e->recs_used = 0;
    return LOCO_OK;
}

int loco_profile_reset(loco_encoder* e) {
    if (!e) return fail(LOCO_E_INVALID, "null encoder");
    int rc = drain_records(e);
    if (rc) return rc;
    for (int i = 0; i < K_COUNT; ++i) {
        e->stats[i].launches = 0;
        e->stats[i].ms = e->stats[i].flops = e->stats[i].bytes = 0.0;
    }
    return LOCO_OK;
}

int loco_profile_read(loco_encoder* e, loco_kernel_stat* stats, int max_stats) {
    if (!e || !stats) return fail(LOCO_E_INVALID, "null argument");
    int rc = drain_records(e);
    if (rc) return rc;
    int n = 0;
    for (int i = 0; i < K_COUNT && n < max_stats; ++i)
        if (e->stats[i].launches) stats[n++] = e->stats[i];
    return n;
}

// ---- single operators ------------------------------------------------------------------------------------
int loco_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int32_t dim, float eps,
                      void* stream) {
    if (!x || !gamma || !beta || !y) return fail(LOCO_E_INVALID, "loco_op_layernorm: null argument");
    if (dim != 512 && dim != 768) return fail(LOCO_E_INVALID, "loco_op_layernorm: dim %d not in {512,768}", dim);
    HIP_TRY(launch_layernorm(x, gamma, beta, y, rows, dim, eps, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_gemm(const float* A, int64_t lda, const float* Wt, int64_t ldw, const float* bias, const float* R, int64_t ldr,
                 float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t nb1, int32_t nb2,
                 int64_t sA1, int64_t sA2, int64_t sC1, int64_t sC2, void* stream) {
    if (!A || !Wt || !C) return fail(LOCO_E_INVALID, "loco_op_gemm: null argument");
    if (K % 32 || (lda | ldw) & 3) return fail(LOCO_E_INVALID, "loco_op_gemm: K %% 32 and lda/ldw %% 4 must be 0");
    if (nb1 < 1 || nb2 < 1) return fail(LOCO_E_INVALID, "loco_op_gemm: batch counts must be >= 1");
    GemmArgs a{A, Wt, bias, R, C, M, N, K, lda, ldw, ldc, ldr, nb1, nb2, sA1, sA2, sC1, sC2, epilogue};
    HIP_TRY(launch_gemm(a, (hipStream_t)stream));
    return LOCO_OK;
}

size_t loco_conv0_scratch_bytes(int32_t B) { return conv0_scratch_bytes(B); }

int loco_op_conv0_gn_gelu(const float* wav, int32_t B, int64_t L, const float* w, const float* gn_w, const float* gn_b,
                          float* out, void* scratch, void* stream) {
    if (!wav || !w || !gn_w || !gn_b || !out || !scratch) return fail(LOCO_E_INVALID, "loco_op_conv0_gn_gelu: null argument");
    if (L < 10) return fail(LOCO_E_INVALID, "loco_op_conv0_gn_gelu: L < 10");
    HIP_TRY(launch_conv0_gn_gelu(wav, B, L, w, gn_w, gn_b, out, scratch, 1e-5f, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_frame_counts(const int32_t* mask, int32_t B, int64_t L, int32_t* frames, void* stream) {
    if (!frames || B <= 0) return fail(LOCO_E_INVALID, "loco_op_frame_counts: invalid argument");
    HIP_TRY(launch_frame_counts(mask, B, L, frames, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_pos_conv(const float* h, const float* w_folded, const float* bias, const float* sin_table, const int32_t* frames,
                     float* out, int32_t B, int32_t T, void* stream) {
    if (!h || !w_folded || !bias || !sin_table || !out) return fail(LOCO_E_INVALID, "loco_op_pos_conv: null argument");
    HIP_TRY(launch_pos_conv(h, w_folded, bias, sin_table, frames, out, B, T, (hipStream_t)stream));
    return LOCO_OK;
}


size_t loco_normalize_scratch_bytes(int32_t B) { return B > 0 ? normalize_scratch_bytes(B) : 0; }

int loco_op_normalize_waveform(const float* wav, const int32_t* attention_mask, int32_t B, int64_t L, float padding_value, float* out,
                               void* scratch, size_t scratch_bytes, void* stream) {
    if (!wav || !out || !scratch || B <= 0 || L <= 0) return fail(LOCO_E_INVALID, "loco_op_normalize_waveform: null/invalid argument");
    if (scratch_bytes < normalize_scratch_bytes(B) || (reinterpret_cast<uintptr_t>(scratch) & 7))
        return fail(LOCO_E_WORKSPACE, "loco_op_normalize_waveform: scratch %zu < %zu bytes (or not 8-byte aligned)", scratch_bytes,
                    normalize_scratch_bytes(B));
    HIP_TRY(launch_normalize_waveform(wav, attention_mask, B, L, padding_value, out, scratch, (hipStream_t)stream));
    return LOCO_OK;
}

// ---- sample-rate conversion ("next" row f-4) -----------------------------------------------------------------------------
int loco_resample_design(int32_t sr_in, int32_t sr_out, int32_t* up, int32_t* down, int32_t* taps_per_phase, float* taps_host) {
    if (!up || !down || !taps_per_phase) return fail(LOCO_E_INVALID, "loco_resample_design: null argument");
    int L = 0, M = 0, K = 0;
    const int rc = resample_design(sr_in, sr_out, &L, &M, &K, taps_host);
    if (rc) return fail(LOCO_E_INVALID, "loco_resample_design: unsupported rates %d -> %d Hz", sr_in, sr_out);
    *up = L; *down = M; *taps_per_phase = K;
    return LOCO_OK;
}

int64_t loco_resample_length(int64_t n_in, int32_t up, int32_t down) {
    if (n_in <= 0 || up <= 0 || down <= 0) return 0;
    return (n_in * up + down - 1) / down;  // ceil(n * sr_out / sr_in): librosa.resample's n_samples (+ fix_length)
}

int loco_op_resample(const float* x, int32_t B, int64_t n_in, int64_t x_stride, const float* taps_dev, int32_t up, int32_t down,
                     int32_t taps_per_phase, float* y, int64_t n_out, int64_t y_stride, void* stream) {
    if (!x || !taps_dev || !y) return fail(LOCO_E_INVALID, "loco_op_resample: null argument");
    if (B <= 0 || n_in <= 0 || n_out <= 0 || n_out > loco_resample_length(n_in, up, down) || x_stride < n_in || y_stride < n_out ||
        (reinterpret_cast<uintptr_t>(taps_dev) & 15))
        return fail(LOCO_E_INVALID, "loco_op_resample: invalid shape (n_out must be <= ceil(n_in * up / down); taps 16-byte aligned)");
    HIP_TRY(launch_resample(x, B, n_in, x_stride, taps_dev, up, down, taps_per_phase, y, n_out, y_stride, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_split_f16(const float* x, void* hi, void* lo, int64_t n, void* stream) {
    if (!x || !hi || !lo || n <= 0 || (n & 3)) return fail(LOCO_E_INVALID, "loco_op_split_f16: invalid argument");
    HIP_TRY(launch_split_f16(x, hi, lo, n, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_gemm_f16x3(const void* Ahi, const void* Alo, int64_t lda, const void* Whi, const void* Wlo, int64_t ldw,
                       const float* bias, const float* R, int64_t ldr, float* C, void* Chi, void* Clo, int64_t ldc, int32_t M,
                       int32_t N, int32_t K, int32_t epilogue, int32_t nb1, int32_t nb2, int64_t sA1, int64_t sA2, int64_t sC1,
                       int64_t sC2, void* stream) {
    if (!Ahi || !Alo || !Whi || !Wlo || (!C && !Chi)) return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3: null argument");
    if (K % 32 || (lda | ldw) & 7) return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3: K %% 32 and lda/ldw %% 8 must be 0");
    GemmSplitArgs a{(const _Float16*)Ahi, (const _Float16*)Alo, (const _Float16*)Whi, (const _Float16*)Wlo, bias, R, C,
                    (_Float16*)Chi, (_Float16*)Clo, M, N, K, lda, ldw, ldc, ldr, nb1, nb2, sA1, sA2, sC1, sC2, epilogue};
    HIP_TRY(launch_gemm_split(a, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_permute_conv_k(const float* w, float* out, int32_t N, int32_t taps, int32_t C, void* stream) {
    if (!w || !out) return fail(LOCO_E_INVALID, "loco_op_permute_conv_k: null argument");
    HIP_TRY(launch_permute_conv_k(w, out, N, taps, C, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_conv_gemm_f16x3(const void* Ahi, const void* Alo, int64_t lda, const void* Whi, const void* Wlo, float* C, void* Chi, void* Clo,
                            int32_t Tout, int32_t N, int32_t Cin, int32_t taps, int32_t epilogue, int32_t B, int64_t sA1, void* stream) {
    if (!Ahi || !Alo || !Whi || !Wlo || (!C && !Chi)) return fail(LOCO_E_INVALID, "loco_op_conv_gemm_f16x3: null argument");
    if (taps < 1 || taps > 3 || Cin % 64 || lda & 7) return fail(LOCO_E_INVALID, "loco_op_conv_gemm_f16x3: taps in 1..3, Cin %% 64 and lda %% 8");
    const int K = taps * Cin;
    GemmSplitArgs a{(const _Float16*)Ahi, (const _Float16*)Alo, (const _Float16*)Whi, (const _Float16*)Wlo, nullptr, nullptr, C,
                    (_Float16*)Chi, (_Float16*)Clo, Tout, N, K, lda, K, N, 0, B, 1, sA1, 0, (int64_t)Tout * N, 0, epilogue};
    a.ktaps = taps;
    HIP_TRY(launch_gemm_split(a, (hipStream_t)stream));
    return LOCO_OK;
}

size_t loco_gemm_splitk_bytes(void) { return kSplitKBytes; }

void loco_debug_reload_gemm_knobs(void) {
    reload_gemm_knobs();
    reload_attention_knobs();
}

int loco_op_gemm_f16x3_splitk(const void* Ahi, const void* Alo, int64_t lda, const void* Whi, const void* Wlo, int64_t ldw,
                              const float* bias, const float* R, int64_t ldr, float* C, void* Chi, void* Clo, int64_t ldc, int32_t M,
                              int32_t N, int32_t K, int32_t epilogue, void* splitk_ws, size_t splitk_bytes, void* stream) {
    if (!Ahi || !Alo || !Whi || !Wlo || (!C && !Chi) || !splitk_ws) return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3_splitk: null argument");
    if (K % 32 || (lda | ldw) & 7) return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3_splitk: K %% 32 and lda/ldw %% 8 must be 0");
    if (splitk_bytes < kSplitKBytes) return fail(LOCO_E_WORKSPACE, "loco_op_gemm_f16x3_splitk: workspace %zu < %zu bytes", splitk_bytes, kSplitKBytes);
    GemmSplitArgs a{(const _Float16*)Ahi, (const _Float16*)Alo, (const _Float16*)Whi, (const _Float16*)Wlo, bias, R, C,
                    (_Float16*)Chi, (_Float16*)Clo, M, N, K, lda, ldw, ldc, ldr, 1, 1, 0, 0, 0, 0, epilogue};
    a.splitk_ws = reinterpret_cast<float*>(splitk_ws);
    HIP_TRY(launch_gemm_split(a, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_attention_f16x3(const void* qhi, const void* qlo, const void* khi, const void* klo, const void* vhi, const void* vlo,
                            const float* qp, const int32_t* frames, float* ctx, int32_t B, int32_t T, void* stream) {
    if (!qhi || !qlo || !khi || !klo || !vhi || !vlo || !qp || !ctx) return fail(LOCO_E_INVALID, "loco_op_attention_f16x3: null argument");
    HIP_TRY(launch_attention_f16x3((const _Float16*)qhi, (const _Float16*)qlo, (const _Float16*)khi, (const _Float16*)klo,
                                   (const _Float16*)vhi, (const _Float16*)vlo, qp, frames, nullptr, nullptr, ctx, B, T,
                                   (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_attention_f16x3_pe(const void* qhi, const void* qlo, const void* khi, const void* klo, const void* vhi, const void* vlo,
                               const void* pe_hi, const void* pe_lo, float pe_scale, float* qp_scratch, const int32_t* frames, float* ctx,
                               int32_t B, int32_t T, void* stream) {
    if (!qhi || !qlo || !khi || !klo || !vhi || !vlo || !pe_hi || !pe_lo || !qp_scratch || !ctx)
        return fail(LOCO_E_INVALID, "loco_op_attention_f16x3_pe: null argument");
    HIP_TRY(launch_attention_f16x3((const _Float16*)qhi, (const _Float16*)qlo, (const _Float16*)khi, (const _Float16*)klo,
                                   (const _Float16*)vhi, (const _Float16*)vlo, qp_scratch, frames, nullptr, nullptr, ctx, B, T,
                                   (hipStream_t)stream, (const _Float16*)pe_hi, (const _Float16*)pe_lo, pe_scale));
    return LOCO_OK;
}

int loco_op_attention_probs(const float* qkv, const float* qp, const int32_t* frames, float* probs, int32_t B, int32_t T, void* stream) {
    if (!qkv || !qp || !probs) return fail(LOCO_E_INVALID, "loco_op_attention_probs: null argument");
    HIP_TRY(launch_attention_probs(qkv, nullptr, nullptr, nullptr, nullptr, qp, frames, probs, B, T, 3, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_attention_probs_f16x3(const void* qhi, const void* qlo, const void* khi, const void* klo, const float* qp, const int32_t* frames,
                                  float* probs, int32_t B, int32_t T, int32_t terms, void* stream) {
    if (!qhi || !qlo || !khi || !klo || !qp || !probs) return fail(LOCO_E_INVALID, "loco_op_attention_probs_f16x3: null argument");
    if (terms != 2 && terms != 3) return fail(LOCO_E_INVALID, "loco_op_attention_probs_f16x3: terms must be 2 or 3");
    HIP_TRY(launch_attention_probs(nullptr, (const _Float16*)qhi, (const _Float16*)qlo, (const _Float16*)khi, (const _Float16*)klo, qp,
                                   frames, probs, B, T, terms, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_attention(const float* qkv, const float* qp, const int32_t* frames, float* ctx, int32_t B, int32_t T, void* stream) {
    if (!qkv || !qp || !ctx) return fail(LOCO_E_INVALID, "loco_op_attention: null argument");
    HIP_TRY(launch_attention(qkv, qp, frames, ctx, B, T, (hipStream_t)stream));
    return LOCO_OK;
}

}  // extern "C"

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

#define DEC_TRY(expr)           \
    do {                        \
        const int rc_ = (expr); \
        if (rc_) return rc_;    \
    } while (0)

// what every decoder entry asks of its handle first (dec_check, pool_check)
int dec_handle_check(const loco_encoder* e, const char* fn) {
    if (!e) return fail(LOCO_E_INVALID, "%s: null encoder", fn);
    if (!e->finalized || !e->dec.ready)
        return fail(LOCO_E_STATE, "%s: the handle has no decoder weights (decoder.prenet.*, decoder.wrapped_decoder.*, text_decoder_postnet.*) or "
                                  "loco_finalize_weights has not run", fn);
    return LOCO_OK;
}

int dec_check(const loco_encoder* e, const char* fn, int B, int T, int S, const void* ws, size_t bytes, DecPlan& p) {
    DEC_TRY(dec_handle_check(e, fn));
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
        DEC_TRY(dec_attention(s, q, kHidden, kHidden, cache, ld_self, (long)p.S * ld_self, nullptr, ctx, B, 1, t + 1, 0, scr));
        DEC_TRY(run_skinny(s, ctx, lw.self_out, x0, tmp, B, kHidden, kHidden, kEpiResidual));
        DEC_TRY(run_ln(e, s, tmp, lw.self_ln.w, lw.self_ln.b, x1, B, kHidden));
        DEC_TRY(run_skinny(s, x1, WB{lw.wcq, lw.bcq}, nullptr, q, B, kHidden, kHidden, kEpiNone));
        DEC_TRY(dec_attention(s, q, kHidden, kHidden, F(p.off_cross) + (size_t)l * 2 * kHidden, ld_cross, (long)p.T * ld_cross, I(p.off_frames), ctx, B,
                              1, p.T, 0, scr));
        DEC_TRY(run_skinny(s, ctx, lw.cross_out, x1, tmp, B, kHidden, kHidden, kEpiResidual));
        DEC_TRY(run_ln(e, s, tmp, lw.cross_ln.w, lw.cross_ln.b, x0, B, kHidden));
        DEC_TRY(run_skinny(s, x0, lw.ffn_in, nullptr, ffn, B, kFfn, kHidden, kEpiGelu));
        DEC_TRY(run_skinny(s, ffn, lw.ffn_out, x0, tmp, B, kHidden, kFfn, kEpiResidual));
        DEC_TRY(run_ln(e, s, tmp, lw.final_ln.w, lw.final_ln.b, x0, B, kHidden));
    }
    DEC_TRY(run_skinny(s, x0, WB{d.lm_head, nullptr}, nullptr, logits, B, d.vocab, kHidden, kEpiNone));
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
    DEC_TRY(dec_set_frames(p, ws, enc_frames, s));
    HIP_TRY(launch_dec_begin(I(p.off_tokens), p.B, p.S, kDecStartToken, kDecPadToken, I(p.off_lengths), I(p.off_state), s));
    return dec_cross_kv(e, p, ws, enc_out, s);
}

}  // namespace

int loco_has_decoder(const loco_encoder* e) {
    if (!e) return 0;
    bool any = false;
    (void)decoder_layers_loaded(e, &any);
    return any && decoder_missing(e, nullptr) == 0 ? 1 : 0;  // a complete set of decoder tensors, not a part of one
}

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
    DEC_TRY(dec_set_frames(p, ws, enc_frames, s));
    DEC_TRY(dec_cross_kv(e, p, ws, enc_out, s));
    HIP_TRY(launch_dec_embed(decoder_input_ids, S, d.embed, d.vocab, d.pos_tab, d.pos_rows, x0, B, S, nullptr, s));
    for (int l = 0; l < p.L; ++l) {
        const DecLayerW& lw = d.L[l];
        if (hidden_states) DEC_TRY(run_copy(e, s, hidden_states[l], x0, (size_t)M * kHidden));
        // the self-attention k|v land in the layout the step reads ([layers][B][S][k | v] with S rows per clip here)
        float* cache = F(p.off_self) + (size_t)l * M * ld_self;
        DEC_TRY(run_gemm(e, s, x0, kHidden, lw.wqkv, kHidden, lw.bqkv, nullptr, 0, q, kHidden, M, kHidden, kHidden, kEpiNone));
        DEC_TRY(run_gemm(e, s, x0, kHidden, lw.wqkv + (size_t)kHidden * kHidden, kHidden, lw.bqkv + kHidden, nullptr, 0, cache, ld_self, M, 2 * kHidden,
                         kHidden, kEpiNone));
        DEC_TRY(dec_attention(s, q, kHidden, (long)S * kHidden, cache, ld_self, (long)S * ld_self, nullptr, ctx, B, S, S, 1, scr));
        if (sink.self_attn)
            HIP_TRY(launch_dec_attention_probs(q, kHidden, (long)S * kHidden, cache, ld_self, (long)S * ld_self, nullptr, sink.self_attn[l], B, S, S, 1,
                                               1.0f, s));
        DEC_TRY(run_gemm(e, s, ctx, kHidden, lw.self_out.w, kHidden, lw.self_out.b, x0, kHidden, tmp, kHidden, M, kHidden, kHidden, kEpiResidual));
        DEC_TRY(run_ln(e, s, tmp, lw.self_ln.w, lw.self_ln.b, x1, M, kHidden));
        DEC_TRY(run_gemm(e, s, x1, kHidden, lw.wcq, kHidden, lw.bcq, nullptr, 0, q, kHidden, M, kHidden, kHidden, kEpiNone));
        const float* ck = F(p.off_cross) + (size_t)l * 2 * kHidden;
        DEC_TRY(dec_attention(s, q, kHidden, (long)S * kHidden, ck, ld_cross, (long)T_enc * ld_cross, I(p.off_frames), ctx, B, S, T_enc, 0, scr));
        const bool averaged = sink.mean && sink.heads[l];
        float* pc = sink.cross_attn ? sink.cross_attn[l] : (averaged ? sink.scratch : nullptr);
        if (pc)
            HIP_TRY(launch_dec_attention_probs(q, kHidden, (long)S * kHidden, ck, ld_cross, (long)T_enc * ld_cross, I(p.off_frames), pc, B, S, T_enc, 0,
                                               1.0f, s));
        if (averaged)
            HIP_TRY(launch_dec_attn_mean(pc, sink.mean, B, S, T_enc, sink.heads[l], l == sink.first_layer, l == sink.last_layer,
                                         1.0f / (float)sink.pairs, s));
        if (!logits && !hidden_states && sink.mean && l == sink.last_layer) return LOCO_OK;
        DEC_TRY(run_gemm(e, s, ctx, kHidden, lw.cross_out.w, kHidden, lw.cross_out.b, x1, kHidden, tmp, kHidden, M, kHidden, kHidden, kEpiResidual));
        DEC_TRY(run_ln(e, s, tmp, lw.cross_ln.w, lw.cross_ln.b, x0, M, kHidden));
        DEC_TRY(run_gemm(e, s, x0, kHidden, lw.ffn_in.w, kHidden, lw.ffn_in.b, nullptr, 0, ffn, kFfn, M, kFfn, kHidden, kEpiGelu));
        DEC_TRY(run_gemm(e, s, ffn, kFfn, lw.ffn_out.w, kFfn, lw.ffn_out.b, x0, kHidden, tmp, kHidden, M, kHidden, kFfn, kEpiResidual));
        DEC_TRY(run_ln(e, s, tmp, lw.final_ln.w, lw.final_ln.b, x0, M, kHidden));
    }
    if (hidden_states) DEC_TRY(run_copy(e, s, hidden_states[p.L], x0, (size_t)M * kHidden));
    if (!logits) return LOCO_OK;
    // lm_head: N = vocab (81) is no multiple of the MFMA GEMM's 4-column epilogue; the weight-streaming kernel takes any N, 64 rows per grid row
    return run_skinny(s, x0, WB{d.lm_head, nullptr}, nullptr, logits, M, d.vocab, kHidden, kEpiNone);
}

int dec_forward_entry(const char* fn, loco_encoder* e, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc,
                      const int32_t* decoder_input_ids, int32_t S, float* logits, float* const* hidden_states, float* const* self_attentions,
                      float* const* cross_attentions, void* workspace, size_t workspace_bytes, void* stream) {
    DecPlan p;
    DEC_TRY(dec_check(e, fn, B, T_enc, S, workspace, workspace_bytes, p));
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
    DEC_TRY(dec_check(e, fn, B, T_enc, S, workspace, (size_t)-1, p));  // the size is checked against the alignment's own plan below
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
    DEC_TRY(dec_forward_walk(e, a.dec, ws, enc_out, enc_frames, decoder_input_ids, nullptr, nullptr, sink, s));
    HIP_TRY(launch_dtw_align(sink.mean, T_enc, token_counts, reinterpret_cast<const int32_t*>(ws + a.dec.off_frames), B, S, T_enc, start_frames,
                             end_frames, reinterpret_cast<unsigned char*>(ws + a.off_back), s));
    return LOCO_OK;
}

int loco_decoder_begin(loco_encoder* e, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc, int32_t S_max,
                       void* workspace, size_t workspace_bytes, void* stream) {
    DecPlan p;
    DEC_TRY(dec_check(e, "loco_decoder_begin", B, T_enc, S_max, workspace, workspace_bytes, p));
    if (B > kSkinnyMaxM) return fail(LOCO_E_INVALID, "loco_decoder_begin: %d clips exceed the decode step's limit of %d rows", B, kSkinnyMaxM);
    if (!enc_out) return fail(LOCO_E_INVALID, "loco_decoder_begin: null encoder output");
    return dec_begin(e, p, static_cast<char*>(workspace), enc_out, enc_frames, (hipStream_t)stream);
}

int loco_decoder_step(loco_encoder* e, int32_t B, int32_t T_enc, int32_t S_max, int32_t t, float* logits, void* workspace,
                      size_t workspace_bytes, void* stream) {
    DecPlan p;
    DEC_TRY(dec_check(e, "loco_decoder_step", B, T_enc, S_max, workspace, workspace_bytes, p));
    if (B > kSkinnyMaxM) return fail(LOCO_E_INVALID, "loco_decoder_step: %d clips exceed the decode step's limit of %d rows", B, kSkinnyMaxM);
    if (t < 0 || t + 1 >= S_max) return fail(LOCO_E_INVALID, "loco_decoder_step: step %d writes token %d of a buffer of %d", t, t + 1, S_max);
    return dec_step(e, p, static_cast<char*>(workspace), t, logits, (hipStream_t)stream);
}

int loco_decoder_read_tokens(const loco_encoder* e, int32_t B, int32_t T_enc, int32_t S_max, int32_t* tokens, int32_t* lengths, const void* workspace,
                             size_t workspace_bytes, void* stream) {
    DecPlan p;
    DEC_TRY(dec_check(e, "loco_decoder_read_tokens", B, T_enc, S_max, workspace, workspace_bytes, p));
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
    DEC_TRY(dec_check(e, "loco_decoder_generate", B, T_enc, max_length, workspace, workspace_bytes, p));
    if (B > kSkinnyMaxM) return fail(LOCO_E_INVALID, "loco_decoder_generate: %d clips exceed the decode step's limit of %d rows", B, kSkinnyMaxM);
    if (!enc_out || !tokens_out) return fail(LOCO_E_INVALID, "loco_decoder_generate: null argument");
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    DEC_TRY(dec_begin(e, p, ws, enc_out, enc_frames, s));
    int32_t* host = e->dec.host_state;
    for (int t = 0; t + 1 < max_length; ++t) {
        DEC_TRY(dec_step(e, p, ws, t, step_logits ? step_logits + (size_t)t * B * e->dec.vocab : nullptr, s));
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
    DEC_TRY(dec_handle_check(e, fn));
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
        DEC_TRY(run_skinny(s, ctx, lw.self_out, x0, tmp, B, kHidden, kHidden, kEpiResidual));
        DEC_TRY(run_ln(e, s, tmp, lw.self_ln.w, lw.self_ln.b, x1, B, kHidden));
        DEC_TRY(run_skinny(s, x1, WB{lw.wcq, lw.bcq}, nullptr, q, B, kHidden, kHidden, kEpiNone));
        const float* ck = F(p.off_cross) + (size_t)l * 2 * kHidden;
        HIP_TRY(launch_dec_pool_attention(q, ck, ld_cross, (long)p.T * ld_cross, ck + kHidden, st.cross_count, ctx, B, max_frames, scr, s));
        DEC_TRY(run_skinny(s, ctx, lw.cross_out, x1, tmp, B, kHidden, kHidden, kEpiResidual));
        DEC_TRY(run_ln(e, s, tmp, lw.cross_ln.w, lw.cross_ln.b, x0, B, kHidden));
        DEC_TRY(run_skinny(s, x0, lw.ffn_in, nullptr, ffn, B, kFfn, kHidden, kEpiGelu));
        DEC_TRY(run_skinny(s, ffn, lw.ffn_out, x0, tmp, B, kHidden, kFfn, kEpiResidual));
        DEC_TRY(run_ln(e, s, tmp, lw.final_ln.w, lw.final_ln.b, x0, B, kHidden));
    }
    DEC_TRY(run_skinny(s, x0, WB{d.lm_head, nullptr}, nullptr, logits, B, d.vocab, kHidden, kEpiNone));
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
    DEC_TRY(pool_check(e, "loco_decoder_pool_init", slots, T_cap, S_max, workspace, workspace_bytes, p));
    HIP_TRY(launch_pool_init(pool_state(p, static_cast<char*>(workspace)), (hipStream_t)stream));
    pool_sampled_set(e, workspace, 0);
    return LOCO_OK;
}

int loco_decoder_pool_admit(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t n, const int32_t* slot_ids, const float* enc_out,
                            int64_t clip_stride, const int32_t* enc_rows, const int32_t* enc_frames, const int32_t* caps, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const char* fn = "loco_decoder_pool_admit";
    PoolPlan p;
    DEC_TRY(pool_check(e, fn, slots, T_cap, S_max, workspace, workspace_bytes, p));
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
        DEC_TRY(pool_admit_check(fn, T_cap, S_max, n, i, enc_rows[i], caps[i], clip_stride));
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
        DEC_TRY(run_gemm(e, s, enc_out + (size_t)i * clip_stride, kHidden, e->dec.wckv, kHidden, e->dec.bckv, nullptr, 0,
                         reinterpret_cast<float*>(ws + p.off_cross) + (size_t)slot_ids[i] * T_cap * N, N, enc_rows[i], N, kHidden, kEpiNone));
    HIP_TRY(launch_pool_admit(st, a, enc_frames, kDecStartToken, s));
    pool_sampled_set(e, workspace, pool_sampled_slots(e, workspace) & ~seen);  // these slots are greedy from here on
    return LOCO_OK;
}

int loco_decoder_pool_step(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t max_pos, int32_t max_frames, float* step_logits,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "loco_decoder_pool_step";
    PoolPlan p;
    DEC_TRY(pool_check(e, fn, slots, T_cap, S_max, workspace, workspace_bytes, p));
    DEC_TRY(pool_step_bounds_check(fn, T_cap, S_max, max_pos, max_frames));
    if (pool_sampled_slots(e, workspace))
        return fail(LOCO_E_STATE, "%s: the pool holds slots admitted to sample (mask 0x%llx); step it with loco_decoder_pool_step_sample", fn,
                    pool_sampled_slots(e, workspace));
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const PoolState st = pool_state(p, ws);
    float* logits = step_logits ? step_logits : reinterpret_cast<float*>(ws + p.off_logits);
    DEC_TRY(pool_step_walk(e, p, ws, st, max_pos, max_frames, logits, s));
    HIP_TRY(launch_pool_select(st, logits, e->dec.vocab, kDecEosToken, s));
    return LOCO_OK;
}

int loco_decoder_pool_admit_samples(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t n, int32_t copies, const int32_t* slot_ids,
                                    const float* enc_out, int64_t clip_stride, const int32_t* enc_rows, const int32_t* enc_frames, const int32_t* caps,
                                    const uint32_t* utterances, const uint32_t* hypotheses, const int32_t* greedy, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const char* fn = "loco_decoder_pool_admit_samples";
    PoolPlan p;
    DEC_TRY(pool_check(e, fn, slots, T_cap, S_max, workspace, workspace_bytes, p));
    if (n <= 0 || copies <= 0 || (int64_t)n * copies > slots)
        return fail(LOCO_E_INVALID, "%s: %d clips x %d copies for a pool of %d slots", fn, n, copies, slots);
    if (!slot_ids || !enc_out || !enc_rows || !caps || !utterances || !hypotheses) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (clip_stride < 0 || (clip_stride & 3) || (reinterpret_cast<uintptr_t>(enc_out) & 15))
        return fail(LOCO_E_INVALID, "%s: enc_out and the clip stride must be 16-byte aligned", fn);
    PoolAdmitSamples a{};
    a.n = n * copies, a.copies = copies;
    unsigned long long seen = 0, draws = 0;
    for (int i = 0; i < n; ++i) {
        DEC_TRY(pool_admit_check(fn, T_cap, S_max, n, i, enc_rows[i], caps[i], clip_stride));
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
        DEC_TRY(run_gemm(e, s, enc_out + (size_t)i * clip_stride, kHidden, e->dec.wckv, kHidden, e->dec.bckv, nullptr, 0, first, N, enc_rows[i], N, kHidden,
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
    DEC_TRY(pool_check(e, fn, slots, T_cap, S_max, workspace, workspace_bytes, p));
    DEC_TRY(pool_step_bounds_check(fn, T_cap, S_max, max_pos, max_frames));
    SampleRule rule;
    DEC_TRY(sample_config_check(config, fn, rule));
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const PoolState st = pool_state(p, ws);
    float* logits = step_logits ? step_logits : reinterpret_cast<float*>(ws + p.off_logits);
    DEC_TRY(pool_step_walk(e, p, ws, st, max_pos, max_frames, logits, s));
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
    DEC_TRY(sample_config_check(config, fn, rule));
    HIP_TRY(launch_sample_tokens(logits, (long)ld, M, V, rule, counters, greedy, tokens, keep, uniform, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_decoder_pool_poll(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t* host_block, const void* workspace,
                           size_t workspace_bytes, void* stream) {
    PoolPlan p;
    DEC_TRY(pool_check(e, "loco_decoder_pool_poll", slots, T_cap, S_max, workspace, workspace_bytes, p));
    if (!host_block) return fail(LOCO_E_INVALID, "loco_decoder_pool_poll: null host block");
    HIP_TRY(hipMemcpyAsync(host_block, static_cast<const char*>(workspace) + p.off_poll, (size_t)(4 + 2 * slots) * sizeof(int32_t),
                           hipMemcpyDeviceToHost, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_decoder_pool_read(loco_encoder* e, int32_t slots, int32_t T_cap, int32_t S_max, int32_t slot, int32_t* tokens, const void* workspace,
                           size_t workspace_bytes, void* stream) {
    PoolPlan p;
    DEC_TRY(pool_check(e, "loco_decoder_pool_read", slots, T_cap, S_max, workspace, workspace_bytes, p));
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

// ---- long-form segmentation (segment.hip) ----
void loco_vad_default_params(LocoVadParams* p) {
    if (!p) return;
    *p = LocoVadParams{(uint32_t)sizeof(LocoVadParams), 1, 20.0, 1.0, 0.3, 0.1, 0.2, 0.10, 0.99, 10.0, -60.0, 15.0};
}

int loco_vad_frames(const LocoVadParams* p, int32_t* frames) {
    const char* fn = "loco_vad_frames";
    if (!p || !frames) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (p->struct_size != sizeof(LocoVadParams))
        return fail(LOCO_E_INVALID, "%s: struct_size = %u is not sizeof(LocoVadParams) = %zu", fn, p->struct_size, sizeof(LocoVadParams));
    const struct { const char* name; double v; } all[] = {
        {"max_segment_s", p->max_segment_s}, {"min_segment_s", p->min_segment_s}, {"min_silence_s", p->min_silence_s},
        {"min_speech_s", p->min_speech_s},   {"pad_s", p->pad_s},                 {"noise_quantile", p->noise_quantile},
        {"peak_quantile", p->peak_quantile}, {"margin_db", p->margin_db},         {"abs_floor_db", p->abs_floor_db},
        {"min_dynamic_db", p->min_dynamic_db}};
    for (const auto& f : all)
        if (!std::isfinite(f.v)) return fail(LOCO_E_INVALID, "%s: %s = %g is not finite", fn, f.name, f.v);
    if (p->max_segment_s > LOCO_VAD_MAX_SEGMENT_S)
        return fail(LOCO_E_INVALID, "%s: max_segment_s = %g exceeds %g s, what the decoder's 450 token positions hold at about 15 characters a second",
                    fn, p->max_segment_s, (double)LOCO_VAD_MAX_SEGMENT_S);
    for (int i = 1; i < 5; ++i)
        if (all[i].v < 0.0 || all[i].v > LOCO_VAD_MAX_SEGMENT_S)
            return fail(LOCO_E_INVALID, "%s: %s = %g is outside 0 .. %g s", fn, all[i].name, all[i].v, (double)LOCO_VAD_MAX_SEGMENT_S);
    const auto to_frames = [](double s) { return (int32_t)std::nearbyint(s * 50.0); };  // ties to even, as Python's round()
    const int32_t maxf = to_frames(p->max_segment_s), minf = to_frames(p->min_segment_s), sil = to_frames(p->min_silence_s);
    if (maxf < 2) return fail(LOCO_E_INVALID, "%s: max_segment_s = %g is below 2 frames (0.04 s)", fn, p->max_segment_s);
    if (minf < 1) return fail(LOCO_E_INVALID, "%s: min_segment_s = %g is below one frame (0.02 s)", fn, p->min_segment_s);
    if (minf >= maxf)
        return fail(LOCO_E_INVALID, "%s: min_segment_s = %g is not below max_segment_s = %g: the walk over cuts would make no progress", fn,
                    p->min_segment_s, p->max_segment_s);
    if (sil < 1) return fail(LOCO_E_INVALID, "%s: min_silence_s = %g is below one frame (0.02 s)", fn, p->min_silence_s);
    if (!(p->noise_quantile > 0.0 && p->noise_quantile < 1.0))
        return fail(LOCO_E_INVALID, "%s: noise_quantile = %g is outside (0, 1)", fn, p->noise_quantile);
    if (!(p->peak_quantile > 0.0 && p->peak_quantile < 1.0))
        return fail(LOCO_E_INVALID, "%s: peak_quantile = %g is outside (0, 1)", fn, p->peak_quantile);
    if (p->noise_quantile >= p->peak_quantile)
        return fail(LOCO_E_INVALID, "%s: noise_quantile = %g is not below peak_quantile = %g", fn, p->noise_quantile, p->peak_quantile);
    if (p->margin_db < 0.0) return fail(LOCO_E_INVALID, "%s: margin_db = %g is negative", fn, p->margin_db);
    if (p->min_dynamic_db < 0.0) return fail(LOCO_E_INVALID, "%s: min_dynamic_db = %g is negative", fn, p->min_dynamic_db);
    frames[0] = maxf;
    frames[1] = minf;
    frames[2] = sil;
    frames[3] = to_frames(p->min_speech_s);
    frames[4] = to_frames(p->pad_s);
    return LOCO_OK;
}

size_t loco_vad_workspace_bytes(int64_t F) { return vad_workspace_bytes((long)F); }

int loco_op_frame_energy_db(const float* wav, int64_t n, float* db, void* stream) {
    const char* fn = "loco_op_frame_energy_db";
    if (!wav || !db) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (n < kVadWindow) return fail(LOCO_E_INVALID, "%s: n = %lld samples is shorter than one frame (400)", fn, (long long)n);
    if (loco_output_frames(n) > kVadMaxFrames)
        return fail(LOCO_E_INVALID, "%s: n = %lld samples exceed %ld frames", fn, (long long)n, kVadMaxFrames);
    HIP_TRY(launch_frame_energy_db(wav, (long)n, db, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_vad_segments(const float* db, int64_t F, const LocoVadParams* params, int32_t* seg_start, int32_t* seg_end, int32_t max_segments,
                         int32_t* count, float* threshold_db, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "loco_op_vad_segments";
    if (!db || !params || !seg_start || !seg_end || !count || !threshold_db || !workspace) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (F < 1 || F > kVadMaxFrames) return fail(LOCO_E_INVALID, "%s: F = %lld is outside 1 .. %ld frames", fn, (long long)F, kVadMaxFrames);
    if (max_segments < 1) return fail(LOCO_E_INVALID, "%s: max_segments = %d must be >= 1", fn, max_segments);
    int32_t fr[5];
    if (const int rc = loco_vad_frames(params, fr)) return rc;
    if (workspace_bytes < vad_workspace_bytes((long)F))
        return fail(LOCO_E_INVALID, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, vad_workspace_bytes((long)F));
    const auto rank = [F](double q) {
        const int64_t k = (int64_t)std::ceil(q * (double)F);
        return (int)(k < 1 ? 1 : (k > F ? F : k));
    };
    VadArgs a{(int)F, fr[0], fr[1], fr[2], fr[3], fr[4], params->trim ? 1 : 0, rank(params->noise_quantile), rank(params->peak_quantile),
              (float)params->margin_db, (float)params->abs_floor_db, (float)params->min_dynamic_db, max_segments};
    HIP_TRY(launch_vad_segments(db, a, seg_start, seg_end, count, threshold_db, workspace, (hipStream_t)stream));
    return LOCO_OK;
}
