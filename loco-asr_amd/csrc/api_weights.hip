// C ABI (include/loco_asr.h), weights: which keys a handle expects and with what shapes (encoder, text prenet, decoder),
// loco_set_weight / loco_missing_weights / loco_has_decoder, and loco_finalize_weights, which binds every tensor a forward reads and
// prepares what the kernels want (fused q|k|v, folded positional conv, fp16 hi/lo planes, the weight-determined range check).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "loco_host.h"

using namespace loco;
using namespace loco::host;

namespace loco::host {

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

}  // namespace loco::host

namespace {

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

}  // namespace

namespace loco::host {

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

}  // namespace loco::host

namespace {

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

extern "C" {

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

int loco_has_decoder(const loco_encoder* e) {
    if (!e) return 0;
    bool any = false;
    (void)decoder_layers_loaded(e, &any);
    return any && decoder_missing(e, nullptr) == 0 ? 1 : 0;  // a complete set of decoder tensors, not a part of one
}

}  // extern "C"
