// C ABI (include/loco_asr.h), the handle itself: the error string every API file reports through, loco_create / loco_destroy, the
// plain setters and getters (precision, streams, taps, attention outputs, range policy), the readers of a forward's status block,
// and profiling (kKernelNames: the buckets loco_profile_read reports).  Weights are api_weights.hip, the forwards api_forward.hip,
// the text decoder api_decoder.hip, the operators that take no handle api_ops.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "loco_host.h"

using namespace loco;
using namespace loco::host;

namespace {

thread_local std::string g_err;

}  // namespace

namespace loco {
int api_fail(int code, const char* fmt, ...) {  // declared in loco_kernels.h: every API file reports through it (fail, loco_host.h)
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

// the KernelId buckets (loco_host.h) by name, in the enum's order
const char* const kKernelNames[K_COUNT] = {"gemm_f32",     "attention_f32", "layernorm",       "conv0_gn_gelu",
                                           "pos_conv_f32", "frame_counts",  "copy",            "gemm_f16x3",
                                           "attention_f16x3", "pos_conv_f16x3_gemm", "attention_probs"};

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

// ---- forwards in flight: one status block per forward (include/loco_asr.h) ---------------------------------------------------
size_t loco_status_bytes(void) { return sizeof(StatusBlock); }

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

}  // extern "C"
