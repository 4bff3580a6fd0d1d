// Host side of the C ABI (include/loco_asr.h): what at least two of the API files -- loco_api.hip, api_weights.hip, api_forward.hip,
// api_decoder.hip, api_ops.hip, lm_api.hip -- need of each other.  Host-only: no kernel file includes this.  Whatever one file alone
// uses (its plans, its workspace carve, its checks) stays in that file's anonymous namespace.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/loco_asr.h"
#include "loco_kernels.h"

// every HIP call of the API: a failure becomes LOCO_E_HIP with the call's text in loco_last_error
#define HIP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return loco::api_fail(LOCO_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// every call that returns a LOCO_* code: the first failure is the caller's result (its error text is already set)
#define LOCO_TRY(expr)          \
    do {                        \
        const int rc_ = (expr); \
        if (rc_) return rc_;    \
    } while (0)

// Nothing below is part of the library's ABI: hidden, so that calls between the API files bind inside the library (no PLT, as when
// all of this was one file's anonymous namespace) and no internal name is exported.
#pragma GCC visibility push(hidden)

namespace loco::host {

inline constexpr auto& fail = loco::api_fail;

inline constexpr int kConvK[7] = {10, 3, 3, 3, 3, 2, 2};
inline constexpr int kConvS[7] = {5, 2, 2, 2, 2, 2, 2};

inline size_t align_up(size_t n) { return (n + 255) & ~size_t(255); }

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

constexpr float kRangeHi = 65504.0f;   // fp16 maximum: hi = fp16(x) is inf from 65520 on
constexpr float kRangeLo = 0.015625f;  // 2^-6: a plane tensor whose LARGEST element is below this has lost fp32-class accuracy

}  // namespace loco::host

// An n-gram language model (loco_ngram_create, ngram_api.hip): the device table and what it was built from
struct loco_ngram {
    loco::NgramTable table{};
    uint64_t* keys = nullptr;  // device, table.mask + 1 slots
    double* vals = nullptr;    // device, [slots][2]
    int64_t grams = 0;
    int device = 0;
};

struct loco_encoder {
    loco_config cfg;
    int device = 0;
    std::map<std::string, float*> raw;  // device copies as loaded, HF names
    std::map<std::string, std::vector<int64_t>> expected;
    bool finalized = false;
    // prepared
    float* conv_w[7] = {nullptr};  // [512, k*512] tap-major (layer 0 stays [512,10])
    float* pos_w = nullptr;        // [16][128][48][48]
    loco::host::SplitW conv_s[7];  // split copies of conv_w[1..6]
    loco::host::SplitW proj_s;     // feature projection
    loco::host::SplitW pe_s;       // relative-position table pe_k [320,64]
    loco::host::SplitW posg_s;     // positional conv weight as the GEMM's W: [16][48][128*48]
    int precision = 1;             // 0 = exact fp32 MFMA, 1 = fp16 x3 split MFMA (default), 2 = f16x2 (weights rounded to fp16; opt-in)
    std::vector<loco::host::LayerW> layers;
    loco::host::StemW stem;
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
    loco::host::DecoderW dec;     // text decoder (optional)
    // decoder pools that hold slots which sample: (workspace, bit r = slot r draws).  On the host because loco_decoder_pool_admit and
    // loco_decoder_pool_step enqueue what they always did: neither can mark a slot on the device.  Single caller, as the pool itself.
    std::vector<std::pair<const void*, unsigned long long>> pool_sampled;
    // decoder pools whose slots are beam groups: (workspace, the config of loco_decoder_pool_admit_beams), kept like pool_sampled
    std::vector<std::pair<const void*, loco_beam_config>> pool_beam;
    // beam pools with an n-gram model attached (loco_decoder_pool_attach_ngram): kept per workspace address, forgotten with the config
    struct PoolFusion {
        const void* ws;
        const loco_ngram* lm;
        double weight, token_bonus;
    };
    std::vector<PoolFusion> pool_fusion;
    std::map<std::string, std::vector<int64_t>> dec_shapes;  // shapes of the decoder tensors as loaded (the vocabulary is theirs)
    // concurrency inside one forward: a batch may run as two half-batches on two streams (loco_set_streams).  The side stream and
    // its events are created on first use under side_mu; forwards in flight together serialise their second halves on it.
    int streams = 2;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::mutex side_mu;
    // range tracking of the fp16-plane activations (loco_kernels.h, range_commit): one status word x 8 shards per stage, in the
    // workspace of each forward; `own` is the status block of the forwards enqueued through loco_forward (pinned host memory)
    loco::host::StatusBlock* own = nullptr;
    float* absmax_dev = nullptr;  // one float, weight preparation
    bool debug_nonfinite = false;                 // LOCO_DEBUG_NONFINITE=1 at loco_create (dbg_check)
    unsigned long long* debug_counter = nullptr;  // two words, device
    int range_policy = 1;         // loco_forward_checked: 1 = re-run out-of-range batches on the exact-fp32 kernels, 0 = report
    std::string range_static;     // non-empty: a weight-determined plane tensor (a LayerNorm output) leaves the range
    // profiling
    bool profiling = false;
    int profile_only = -1;  // >= 0: only launches of this kernel bucket are bracketed (loco_set_profiling_filter)
    std::vector<loco::host::ProfRec> recs;
    size_t recs_used = 0;
    loco_kernel_stat stats[loco::host::K_COUNT];
};

namespace loco::host {

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
inline double gemm_flops(int M, int N, int K, int nb1, int nb2) { return 2.0 * M * (double)N * K * ((double)nb1 * nb2); }
inline double gemm_bytes(int M, int N, int K, int nb1, int nb2, int epi) {
    const double nb = (double)nb1 * nb2;
    return 4.0 * (nb * ((double)M * K + (double)M * N * (epi == kEpiResidual ? 2 : 1)) + (double)N * K);
}

inline int run_gemm(loco_encoder* e, hipStream_t s, const float* A, long lda, const float* Wt, long ldw, const float* bias,
                    const float* R, long ldr, float* C, long ldc, int M, int N, int K, int epi, int nb1 = 1, int nb2 = 1,
                    long sA1 = 0, long sA2 = 0, long sC1 = 0, long sC2 = 0) {
    GemmArgs a{A, Wt, bias, R, C, M, N, K, lda, ldw, ldc, ldr, nb1, nb2, sA1, sA2, sC1, sC2, epi};
    Bracket br(e, s, K_GEMM, gemm_flops(M, N, K, nb1, nb2), gemm_bytes(M, N, K, nb1, nb2, epi));
    HIP_TRY(launch_gemm(a, s));
    return LOCO_OK;
}

inline int run_ln(loco_encoder* e, hipStream_t s, const float* x, const float* g, const float* b, float* y, long rows, int dim,
                  _Float16* yhi = nullptr, _Float16* ylo = nullptr, float* nonfinite_slot = nullptr, const _Float16* rhi = nullptr,
                  const _Float16* rlo = nullptr) {
    Bracket br(e, s, K_LN, (rhi ? 10.0 : 8.0) * rows * dim, ((y && yhi ? 12.0 : 8.0) + (rhi ? 4.0 : 0.0)) * rows * dim);
    HIP_TRY(launch_layernorm(x, g, b, y, rows, dim, e->cfg.ln_eps, s, yhi, ylo, nonfinite_slot, rhi, rlo));
    return LOCO_OK;
}

inline int run_copy(loco_encoder* e, hipStream_t s, float* dst, const float* src, size_t n) {
    Bracket br(e, s, K_COPY, 0.0, 8.0 * n);
    HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return LOCO_OK;
}

// defined in api_weights.hip
void build_expected(loco_encoder* e);                           // the encoder's keys and shapes (loco_create)
int decoder_layers_loaded(const loco_encoder* e, bool* any);    // decoder layer count of the tensors loaded so far
// defined in api_forward.hip
int ensure_sin_rows(loco_encoder* e, int rows, hipStream_t s, const float** tab);  // the sinusoid table, grown on demand

}  // namespace loco::host

#pragma GCC visibility pop
