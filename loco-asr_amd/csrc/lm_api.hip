// C ABI of the GPT-2 language-model scorer (include/loco_asr.h, "language model"): the handle, the two forward functions and the
// operators of the parity tests.  The layer body is launch_layernorm / launch_gemm / launch_dec_attention as they stand; lm.hip has the
// embedding, the row gather and the fused LM head.  Forwards allocate nothing, never synchronise and run on the caller's stream.
// The cached-context half (loco_lm_cache_*, loco_lm_ctx_step) runs the same body with lm_attention.hip's prefix + causal attention.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "loco_host.h"

using namespace loco;
using namespace loco::host;

namespace {

struct LmLayerW {
    const float *ln1_w = nullptr, *ln1_b = nullptr, *ln2_w = nullptr, *ln2_b = nullptr;
    const float *bqkv = nullptr, *bo = nullptr, *bfc = nullptr, *bproj = nullptr;
    float *wqkv = nullptr, *wo = nullptr, *wfc = nullptr, *wproj = nullptr;  // [N, K], transposed from HF's Conv1D [in, out] at finalize
};

struct Expect {
    long d0, d1;  // d1 == 0: one-dimensional
};

}  // namespace

struct loco_lm {
    int n_layer = 0, n_positions = 0, vocab = 0, ldv = 0;
    bool ready = false;
    std::map<std::string, Expect> expect;
    std::map<std::string, float*> raw;
    std::vector<LmLayerW> L;
    const float *wte = nullptr, *wpe = nullptr, *lnf_w = nullptr, *lnf_b = nullptr;
};

namespace {

struct LmWorkspace {
    int32_t* status;
    float *x, *ln, *qkv, *ffn, *attn, *hsel;
    int32_t* targets;
    void* part;
    size_t bytes;
};

LmWorkspace carve(const loco_lm* lm, void* base, int B, int S, int R) {
    char* p = static_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t n) {
        char* q = p + off;
        off += align_up(n);
        return q;
    };
    const size_t rows = (size_t)B * S;
    LmWorkspace w;
    w.status = reinterpret_cast<int32_t*>(take(256));
    w.x = reinterpret_cast<float*>(take(rows * kHidden * sizeof(float)));
    w.ln = reinterpret_cast<float*>(take(rows * kHidden * sizeof(float)));  // LayerNorm output, then the attention context
    w.qkv = reinterpret_cast<float*>(take(rows * kQkv * sizeof(float)));
    w.ffn = reinterpret_cast<float*>(take(rows * kFfn * sizeof(float)));
    w.attn = reinterpret_cast<float*>(take(dec_attention_scratch_bytes(B, S, S)));
    w.hsel = reinterpret_cast<float*>(take((size_t)R * kHidden * sizeof(float)));
    w.targets = reinterpret_cast<int32_t*>(take((size_t)R * sizeof(int32_t)));
    w.part = take(lm_head_scratch_bytes(R, lm->vocab));
    w.bytes = off;
    return w;
}

int check_shape(const loco_lm* lm, const char* fn, int B, int S) {
    if (!lm) return api_fail(LOCO_E_INVALID, "%s: null handle", fn);
    if (!lm->ready) return api_fail(LOCO_E_STATE, "%s: weights not finalized (loco_lm_finalize)", fn);
    if (B < 1 || B > 65535) return api_fail(LOCO_E_INVALID, "%s: B = %d is outside 1 .. 65535", fn, B);
    if (S < 1 || S > lm->n_positions) return api_fail(LOCO_E_INVALID, "%s: S = %d is outside 1 .. n_positions = %d", fn, S, lm->n_positions);
    if ((long)B * S > (1L << 24)) return api_fail(LOCO_E_INVALID, "%s: B * S = %ld rows are too many for one call", fn, (long)B * S);
    return LOCO_OK;
}

// embedding and the n_layer pre-LN blocks: w.x = the residual stream before ln_f.  hidden (optional): n_layer + 1 device pointers
int lm_body(const loco_lm* lm, const int32_t* tokens, const int32_t* starts, const int32_t* lens, int B, int S, const LmWorkspace& w,
            float* const* hidden, hipStream_t st) {
    const int M = B * S;
    const size_t row_bytes = (size_t)M * kHidden * sizeof(float);
    HIP_TRY(hipMemsetAsync(w.status, 0x7f, 256, st));
    HIP_TRY(launch_lm_embed(tokens, starts, lens, lm->wte, lm->vocab, lm->wpe, w.x, B, S, w.status, st));
    if (hidden && hidden[0]) HIP_TRY(hipMemcpyAsync(hidden[0], w.x, row_bytes, hipMemcpyDeviceToDevice, st));
    auto gemm = [&](const float* A, const float* W, const float* bias, const float* R, float* C, int N, int K, int epi) {
        GemmArgs a{A, W, bias, R, C, M, N, K, K, K, N, N, 1, 1, 0, 0, 0, 0, epi};
        return launch_gemm(a, st);
    };
    for (int l = 0; l < lm->n_layer; ++l) {
        const LmLayerW& W = lm->L[l];
        HIP_TRY(launch_layernorm(w.x, W.ln1_w, W.ln1_b, w.ln, M, kHidden, 1e-5f, st));
        HIP_TRY(gemm(w.ln, W.wqkv, W.bqkv, nullptr, w.qkv, kQkv, kHidden, kEpiNone));
        // causal, key counts lens[b], scale 1/8, no bias table; right padding needs no other mask
        HIP_TRY(launch_dec_attention(w.qkv, kQkv, (long)S * kQkv, w.qkv + kHidden, kQkv, (long)S * kQkv, w.qkv + 2 * kHidden, kQkv, (long)S * kQkv, lens,
                                        w.ln, kHidden, (long)S * kHidden, B, S, S, 1, 0, 0.125f, w.attn, st));
        HIP_TRY(gemm(w.ln, W.wo, W.bo, w.x, w.x, kHidden, kHidden, kEpiResidual));
        HIP_TRY(launch_layernorm(w.x, W.ln2_w, W.ln2_b, w.ln, M, kHidden, 1e-5f, st));
        HIP_TRY(gemm(w.ln, W.wfc, W.bfc, nullptr, w.ffn, kFfn, kHidden, kEpiGeluNew));
        HIP_TRY(gemm(w.ffn, W.wproj, W.bproj, w.x, w.x, kHidden, kFfn, kEpiResidual));
        if (hidden && l + 1 < lm->n_layer && hidden[l + 1]) HIP_TRY(hipMemcpyAsync(hidden[l + 1], w.x, row_bytes, hipMemcpyDeviceToDevice, st));
    }
    return LOCO_OK;
}

}  // namespace

// K/V cache of the cached-context forward: per slot and layer n_positions rows of k and of v, and per slot the residual row of its last
// token (what predicts the next one).  `length` is host-side state: it changes when a step is ENQUEUED, so calls on one stream see each
// other's commits in order.
struct loco_lm_cache {
    loco_lm* lm = nullptr;
    int slots = 0;
    float *k = nullptr, *v = nullptr;  // [n_layer][slots][n_positions][768] each
    float* last = nullptr;             // [slots][768]
    std::vector<int32_t> length;
};

namespace {

struct LmCtxWorkspace {
    int32_t* status;
    float *x, *ln, *qkv, *ffn, *hsel;
    int32_t* targets;
    void* part;
    size_t bytes;
};

LmCtxWorkspace carve_ctx(const loco_lm* lm, void* base, int rows) {
    char* p = static_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t n) {
        char* q = p + off;
        off += align_up(n);
        return q;
    };
    LmCtxWorkspace w;
    w.status = reinterpret_cast<int32_t*>(take(256));
    w.x = reinterpret_cast<float*>(take((size_t)rows * kHidden * sizeof(float)));
    w.ln = reinterpret_cast<float*>(take((size_t)rows * kHidden * sizeof(float)));  // LayerNorm output, then the attention context
    w.qkv = reinterpret_cast<float*>(take((size_t)rows * kQkv * sizeof(float)));
    w.ffn = reinterpret_cast<float*>(take((size_t)rows * kFfn * sizeof(float)));
    w.hsel = reinterpret_cast<float*>(take((size_t)rows * kHidden * sizeof(float)));  // at most every row is scored
    w.targets = reinterpret_cast<int32_t*>(take((size_t)rows * sizeof(int32_t)));
    w.part = take(lm_head_scratch_bytes(rows, lm->vocab));
    w.bytes = off;
    return w;
}

constexpr int kLmCtxMaxRows = kLmCtxMaxSeqs * LOCO_LM_MAX_POSITIONS;

}  // namespace

extern "C" {

loco_lm_cache* loco_lm_cache_create(loco_lm* lm, int32_t slots) {
    const char* fn = "loco_lm_cache_create";
    if (!lm) {
        api_fail(LOCO_E_INVALID, "%s: null handle", fn);
        return nullptr;
    }
    if (slots < 1 || slots > LOCO_LM_CACHE_MAX_SLOTS) {
        api_fail(LOCO_E_INVALID, "%s: slots = %d is outside 1 .. %d", fn, slots, LOCO_LM_CACHE_MAX_SLOTS);
        return nullptr;
    }
    loco_lm_cache* c = new loco_lm_cache;
    c->lm = lm, c->slots = slots;
    c->length.assign(slots, 0);
    const size_t plane = (size_t)lm->n_layer * slots * lm->n_positions * kHidden * sizeof(float);
    if (hipMalloc(reinterpret_cast<void**>(&c->k), plane) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&c->v), plane) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->last), (size_t)slots * kHidden * sizeof(float)) != hipSuccess) {
        api_fail(LOCO_E_HIP, "%s: hipMalloc of 2 x %zu bytes failed", fn, plane);
        loco_lm_cache_destroy(c);
        return nullptr;
    }
    return c;
}

void loco_lm_cache_destroy(loco_lm_cache* c) {
    if (!c) return;
    for (float* p : {c->k, c->v, c->last})
        if (p) (void)hipFree(p);
    delete c;
}

int loco_lm_cache_reset(loco_lm_cache* c, int32_t slot) {
    if (!c) return api_fail(LOCO_E_INVALID, "loco_lm_cache_reset: null handle");
    if (slot < 0 || slot >= c->slots) return api_fail(LOCO_E_INVALID, "loco_lm_cache_reset: slot = %d is outside 0 .. %d", slot, c->slots - 1);
    c->length[slot] = 0;
    return LOCO_OK;
}

int32_t loco_lm_cache_length(loco_lm_cache* c, int32_t slot) { return c && slot >= 0 && slot < c->slots ? c->length[slot] : -1; }

size_t loco_lm_ctx_workspace_bytes(loco_lm* lm, int32_t rows, int32_t N) {
    if (!lm || N < 1 || N > kLmCtxMaxSeqs || rows < N || rows > kLmCtxMaxRows || (long)rows > (long)N * lm->n_positions) return 0;
    return carve_ctx(lm, nullptr, rows).bytes;
}

int loco_lm_ctx_step(loco_lm* lm, loco_lm_cache* cache, const int32_t* tokens, const int32_t* seqs, int32_t N, float* nll_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    const char* fn = "loco_lm_ctx_step";
    if (!lm || !cache || !tokens || !seqs || !workspace) return api_fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (cache->lm != lm) return api_fail(LOCO_E_INVALID, "%s: the cache belongs to another model handle", fn);
    if (!lm->ready) return api_fail(LOCO_E_STATE, "%s: weights not finalized (loco_lm_finalize)", fn);
    if (N < 1 || N > kLmCtxMaxSeqs) return api_fail(LOCO_E_INVALID, "%s: N = %d is outside 1 .. %d", fn, N, kLmCtxMaxSeqs);
    LmCtxSeqs s{};
    s.n = N;
    int rows = 0, R = 0;
    unsigned long long committing = 0;
    for (int n = 0; n < N; ++n) {
        const int32_t start = seqs[4 * n], len = seqs[4 * n + 1], slot = seqs[4 * n + 2], flags = seqs[4 * n + 3];
        if (slot < 0 || slot >= cache->slots) return api_fail(LOCO_E_INVALID, "%s: sequence %d: slot = %d is outside 0 .. %d", fn, n, slot, cache->slots - 1);
        if (len < 1) return api_fail(LOCO_E_INVALID, "%s: sequence %d: len = %d must be >= 1", fn, n, len);
        if (start < 0) return api_fail(LOCO_E_INVALID, "%s: sequence %d: start = %d is negative", fn, n, start);
        if (flags & ~(LOCO_LM_CTX_SCORE | LOCO_LM_CTX_COMMIT) || !flags)
            return api_fail(LOCO_E_INVALID, "%s: sequence %d: flags = %d must be SCORE (1), COMMIT (2) or both", fn, n, flags);
        const int P = cache->length[slot];
        if (P + len > lm->n_positions)
            return api_fail(LOCO_E_INVALID, "%s: sequence %d: P + len = %d + %d exceeds n_positions = %d (slot %d)", fn, n, P, len, lm->n_positions, slot);
        if (flags & LOCO_LM_CTX_COMMIT) {
            if (committing >> slot & 1) return api_fail(LOCO_E_INVALID, "%s: sequence %d: two committing sequences on slot %d in one call", fn, n, slot);
            committing |= 1ull << slot;
        }
        s.row0[n] = rows, s.len[n] = len, s.slot[n] = slot, s.P[n] = P, s.tok0[n] = start, s.flags[n] = flags;
        rows += len;
        if (flags & LOCO_LM_CTX_SCORE) R += len;
    }
    if (R && !nll_out) return api_fail(LOCO_E_INVALID, "%s: null nll_out with a scoring sequence", fn);
    const LmCtxWorkspace w = carve_ctx(lm, workspace, rows);
    if (workspace_bytes < w.bytes) return api_fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    const long slot_stride = (long)lm->n_positions * kHidden, layer_stride = slot_stride * cache->slots;
    HIP_TRY(hipMemsetAsync(w.status, 0x7f, 256, st));
    HIP_TRY(launch_lm_ctx_embed(tokens, s, lm->wte, lm->vocab, lm->wpe, w.x, w.status, st));
    auto gemm = [&](const float* A, const float* W, const float* bias, const float* R_, float* C, int Nn, int K, int epi) {
        GemmArgs a{A, W, bias, R_, C, rows, Nn, K, K, K, Nn, Nn, 1, 1, 0, 0, 0, 0, epi};
        return launch_gemm(a, st);
    };
    for (int l = 0; l < lm->n_layer; ++l) {
        const LmLayerW& W = lm->L[l];
        float *kc = cache->k + l * layer_stride, *vc = cache->v + l * layer_stride;
        HIP_TRY(launch_layernorm(w.x, W.ln1_w, W.ln1_b, w.ln, rows, kHidden, 1e-5f, st));
        HIP_TRY(gemm(w.ln, W.wqkv, W.bqkv, nullptr, w.qkv, kQkv, kHidden, kEpiNone));
        HIP_TRY(launch_lm_ctx_attention(w.qkv, kc, vc, slot_stride, s, w.ln, st));
        if (committing) HIP_TRY(launch_lm_ctx_append(w.qkv, s, kc, vc, slot_stride, st));  // rows >= P: nothing this layer's attention read
        HIP_TRY(gemm(w.ln, W.wo, W.bo, w.x, w.x, kHidden, kHidden, kEpiResidual));
        HIP_TRY(launch_layernorm(w.x, W.ln2_w, W.ln2_b, w.ln, rows, kHidden, 1e-5f, st));
        HIP_TRY(gemm(w.ln, W.wfc, W.bfc, nullptr, w.ffn, kFfn, kHidden, kEpiGeluNew));
        HIP_TRY(gemm(w.ffn, W.wproj, W.bproj, w.x, w.x, kHidden, kFfn, kEpiResidual));
    }
    if (R) {  // only the scored rows go through ln_f and the head; the slots' last rows are read before a commit replaces them
        HIP_TRY(launch_lm_ctx_gather(w.x, tokens, s, cache->last, R, LOCO_LM_IGNORE_INDEX, w.hsel, w.targets, st));
        HIP_TRY(launch_layernorm(w.hsel, lm->lnf_w, lm->lnf_b, w.hsel, R, kHidden, 1e-5f, st));
        HIP_TRY(launch_lm_head_nll(w.hsel, kHidden, lm->wte, kHidden, w.targets, R, lm->vocab, LOCO_LM_IGNORE_INDEX, nll_out, w.part, st));
    }
    if (committing) {
        HIP_TRY(launch_lm_ctx_last(w.x, s, cache->last, st));
        for (int n = 0; n < N; ++n)
            if (s.flags[n] & LOCO_LM_CTX_COMMIT) cache->length[s.slot[n]] += s.len[n];
    }
    return LOCO_OK;
}

int loco_op_lm_ctx_attention(const float* qkv, const float* kcache, const float* vcache, int64_t slot_stride, const int32_t* seqs, int32_t N,
                             int32_t slots, float* out, void* stream) {
    const char* fn = "loco_op_lm_ctx_attention";
    if (!qkv || !kcache || !vcache || !seqs || !out) return api_fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (N < 1 || N > kLmCtxMaxSeqs) return api_fail(LOCO_E_INVALID, "%s: N = %d is outside 1 .. %d", fn, N, kLmCtxMaxSeqs);
    if (slots < 1 || slot_stride < kHidden || slot_stride % kHidden) return api_fail(LOCO_E_INVALID, "%s: slots = %d, slot_stride = %lld: need slots >= 1 and a stride of whole rows of 768", fn, slots, (long long)slot_stride);
    LmCtxSeqs s{};
    s.n = N;
    int rows = 0;
    for (int n = 0; n < N; ++n) {
        const int32_t len = seqs[3 * n], slot = seqs[3 * n + 1], P = seqs[3 * n + 2];
        if (len < 1 || len > LOCO_LM_MAX_POSITIONS) return api_fail(LOCO_E_INVALID, "%s: sequence %d: len = %d is outside 1 .. %d", fn, n, len, LOCO_LM_MAX_POSITIONS);
        if (slot < 0 || slot >= slots) return api_fail(LOCO_E_INVALID, "%s: sequence %d: slot = %d is outside 0 .. %d", fn, n, slot, slots - 1);
        if (P < 0 || (long)P * kHidden > slot_stride) return api_fail(LOCO_E_INVALID, "%s: sequence %d: P = %d does not fit the slot's %lld rows", fn, n, P, (long long)(slot_stride / kHidden));
        s.row0[n] = rows, s.len[n] = len, s.slot[n] = slot, s.P[n] = P;
        rows += len;
    }
    HIP_TRY(launch_lm_ctx_attention(qkv, kcache, vcache, (long)slot_stride, s, out, (hipStream_t)stream));
    return LOCO_OK;
}

loco_lm* loco_lm_create(int32_t n_layer, int32_t n_positions, int32_t vocab, int32_t n_embd, int32_t n_head) {
    if (n_embd != kHidden) {
        api_fail(LOCO_E_INVALID, "loco_lm_create: n_embd = %d is not supported: only 768 (checkpoint \"gpt2\"; gpt2-medium, -large and -xl are out of scope)",
                 n_embd);
        return nullptr;
    }
    if (n_head != kHeads) {
        api_fail(LOCO_E_INVALID, "loco_lm_create: n_head = %d is not supported: only 12 heads of 64 (checkpoint \"gpt2\")", n_head);
        return nullptr;
    }
    if (n_layer < 1 || n_layer > 48) {
        api_fail(LOCO_E_INVALID, "loco_lm_create: n_layer = %d is outside 1 .. 48", n_layer);
        return nullptr;
    }
    if (n_positions < 1 || n_positions > LOCO_LM_MAX_POSITIONS) {
        api_fail(LOCO_E_INVALID, "loco_lm_create: n_positions = %d is outside 1 .. %d", n_positions, LOCO_LM_MAX_POSITIONS);
        return nullptr;
    }
    if (vocab < 1 || vocab > (1 << 24)) {
        api_fail(LOCO_E_INVALID, "loco_lm_create: vocab = %d is outside 1 .. 2^24", vocab);
        return nullptr;
    }
    loco_lm* lm = new loco_lm;
    lm->n_layer = n_layer, lm->n_positions = n_positions, lm->vocab = vocab, lm->ldv = (vocab + 3) & ~3;
    lm->L.resize(n_layer);
    auto& e = lm->expect;
    e["wte.weight"] = {vocab, kHidden};
    e["wpe.weight"] = {n_positions, kHidden};
    e["ln_f.weight"] = {kHidden, 0};
    e["ln_f.bias"] = {kHidden, 0};
    for (int l = 0; l < n_layer; ++l) {
        const std::string p = "h." + std::to_string(l) + ".";
        for (const char* ln : {"ln_1.", "ln_2."}) {
            e[p + ln + "weight"] = {kHidden, 0};
            e[p + ln + "bias"] = {kHidden, 0};
        }
        e[p + "attn.c_attn.weight"] = {kHidden, kQkv};
        e[p + "attn.c_attn.bias"] = {kQkv, 0};
        e[p + "attn.c_proj.weight"] = {kHidden, kHidden};
        e[p + "attn.c_proj.bias"] = {kHidden, 0};
        e[p + "mlp.c_fc.weight"] = {kHidden, kFfn};
        e[p + "mlp.c_fc.bias"] = {kFfn, 0};
        e[p + "mlp.c_proj.weight"] = {kFfn, kHidden};
        e[p + "mlp.c_proj.bias"] = {kHidden, 0};
    }
    return lm;
}

void loco_lm_destroy(loco_lm* lm) {
    if (!lm) return;
    for (auto& kv : lm->raw) (void)hipFree(kv.second);
    for (auto& W : lm->L)
        for (float* p : {W.wqkv, W.wo, W.wfc, W.wproj})
            if (p) (void)hipFree(p);
    delete lm;
}

int loco_lm_set_weight(loco_lm* lm, const char* hf_key, const void* dev_ptr, const int64_t* shape, int ndim) {
    const char* fn = "loco_lm_set_weight";
    if (!lm || !hf_key) return api_fail(LOCO_E_INVALID, "%s: null argument", fn);
    std::string key = hf_key;
    if (key.rfind("transformer.", 0) == 0) key = key.substr(12);
    // the causal mask buffers of older checkpoints and the tied head: nothing to store (the caller checks lm_head.weight against wte)
    const size_t n = key.size();
    if (key == "lm_head.weight" || (n > 10 && key.compare(n - 10, 10, ".attn.bias") == 0) ||
        (n > 17 && key.compare(n - 17, 17, ".attn.masked_bias") == 0))
        return LOCO_OK;
    const auto it = lm->expect.find(key);
    if (it == lm->expect.end()) return api_fail(LOCO_E_INVALID, "%s: unknown key '%s'", fn, hf_key);
    if (!shape) return api_fail(LOCO_E_INVALID, "%s: null shape for '%s'", fn, hf_key);
    const Expect ex = it->second;
    const bool ok = ex.d1 ? (ndim == 2 && shape[0] == ex.d0 && shape[1] == ex.d1) : (ndim == 1 && shape[0] == ex.d0);
    if (!ok) {
        char got[96] = "", *g = got;
        for (int i = 0; i < ndim && i < 4; ++i) g += snprintf(g, got + sizeof got - g, i ? ", %lld" : "%lld", (long long)shape[i]);
        return ex.d1 ? api_fail(LOCO_E_INVALID, "%s: '%s' has shape [%s], expected [%ld, %ld]", fn, hf_key, got, ex.d0, ex.d1)
                     : api_fail(LOCO_E_INVALID, "%s: '%s' has shape [%s], expected [%ld]", fn, hf_key, got, ex.d0);
    }
    if (!dev_ptr) return api_fail(LOCO_E_INVALID, "%s: null data for '%s'", fn, hf_key);  // after the name and the shape: a caller may probe those
    const size_t count = (size_t)ex.d0 * (ex.d1 ? ex.d1 : 1);
    // wte is also loco_lm_forward's GEMM weight, whose N must be a multiple of 4: its buffer has ldv rows, the last up to 3 of them zero
    const size_t alloc = key == "wte.weight" ? (size_t)lm->ldv * kHidden : count;
    float*& buf = lm->raw[key];
    if (!buf) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&buf), alloc * sizeof(float)));
        if (alloc > count) HIP_TRY(hipMemset(buf + count, 0, (alloc - count) * sizeof(float)));
    }
    HIP_TRY(hipMemcpy(buf, dev_ptr, count * sizeof(float), hipMemcpyDeviceToDevice));
    lm->ready = false;
    return LOCO_OK;
}

int loco_lm_missing_weights(loco_lm* lm, char* buf, size_t cap) {
    if (!lm) return api_fail(LOCO_E_INVALID, "loco_lm_missing_weights: null handle");
    int missing = 0;
    std::string names;
    for (const auto& kv : lm->expect)
        if (!lm->raw.count(kv.first) && !(lm->ready && kv.second.d1 && kv.first.rfind("h.", 0) == 0)) {
            names += (missing ? "," : "") + kv.first;
            ++missing;
        }
    if (buf && cap) {
        strncpy(buf, names.c_str(), cap - 1);
        buf[cap - 1] = 0;
    }
    return missing;
}

int loco_lm_finalize(loco_lm* lm, void* stream) {
    const char* fn = "loco_lm_finalize";
    if (!lm) return api_fail(LOCO_E_INVALID, "%s: null handle", fn);
    if (lm->ready) return LOCO_OK;
    char first[200];
    const int missing = loco_lm_missing_weights(lm, first, sizeof first);
    if (missing) return api_fail(LOCO_E_STATE, "%s: %d weights missing: %s", fn, missing, first);
    hipStream_t st = (hipStream_t)stream;
    auto get = [&](const std::string& k) { return lm->raw.at(k); };
    lm->wte = get("wte.weight"), lm->wpe = get("wpe.weight"), lm->lnf_w = get("ln_f.weight"), lm->lnf_b = get("ln_f.bias");
    std::vector<std::string> done;
    for (int l = 0; l < lm->n_layer; ++l) {
        const std::string p = "h." + std::to_string(l) + ".";
        LmLayerW& W = lm->L[l];
        W.ln1_w = get(p + "ln_1.weight"), W.ln1_b = get(p + "ln_1.bias"), W.ln2_w = get(p + "ln_2.weight"), W.ln2_b = get(p + "ln_2.bias");
        W.bqkv = get(p + "attn.c_attn.bias"), W.bo = get(p + "attn.c_proj.bias"), W.bfc = get(p + "mlp.c_fc.bias"), W.bproj = get(p + "mlp.c_proj.bias");
        const struct { const char* name; float** dst; int in, out; } mats[4] = {{"attn.c_attn.weight", &W.wqkv, kHidden, kQkv},
                                                                                 {"attn.c_proj.weight", &W.wo, kHidden, kHidden},
                                                                                 {"mlp.c_fc.weight", &W.wfc, kHidden, kFfn},
                                                                                 {"mlp.c_proj.weight", &W.wproj, kFfn, kHidden}};
        for (const auto& m : mats) {  // HF Conv1D [in, out] -> the GEMM's [N = out, K = in]
            if (!*m.dst) HIP_TRY(hipMalloc(reinterpret_cast<void**>(m.dst), (size_t)m.in * m.out * sizeof(float)));
            HIP_TRY(launch_lm_transpose(get(p + m.name), *m.dst, m.in, m.out, st));
            done.push_back(p + m.name);
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (const auto& k : done) {  // the [in, out] originals are not read again
        (void)hipFree(lm->raw[k]);
        lm->raw.erase(k);
    }
    lm->ready = true;
    return LOCO_OK;
}

int32_t loco_lm_vocab_stride(loco_lm* lm) { return lm ? lm->ldv : 0; }

size_t loco_lm_workspace_bytes(loco_lm* lm, int32_t B, int32_t S, int32_t R) {
    if (!lm || B < 1 || B > 65535 || S < 1 || S > lm->n_positions || R < 0) return 0;
    return carve(lm, nullptr, B, S, R).bytes;
}

int loco_lm_nll(loco_lm* lm, const int32_t* tokens, const int32_t* starts, const int32_t* lens, int32_t B, int32_t S, const int32_t* rows, int32_t R,
                float* nll_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "loco_lm_nll";
    if (const int rc = check_shape(lm, fn, B, S)) return rc;
    if (!tokens || !starts || !lens || !rows || !nll_out || !workspace) return api_fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (R < 1 || (long)R > (long)B * S) return api_fail(LOCO_E_INVALID, "%s: R = %d is outside 1 .. B * S = %ld", fn, R, (long)B * S);
    const LmWorkspace w = carve(lm, workspace, B, S, R);
    if (workspace_bytes < w.bytes) return api_fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = lm_body(lm, tokens, starts, lens, B, S, w, nullptr, st)) return rc;
    // only the rows that are scored go through ln_f and the head
    HIP_TRY(launch_lm_gather(w.x, rows, tokens, starts, lens, B, S, R, LOCO_LM_IGNORE_INDEX, w.hsel, w.targets, st));
    HIP_TRY(launch_layernorm(w.hsel, lm->lnf_w, lm->lnf_b, w.hsel, R, kHidden, 1e-5f, st));
    HIP_TRY(launch_lm_head_nll(w.hsel, kHidden, lm->wte, kHidden, w.targets, R, lm->vocab, LOCO_LM_IGNORE_INDEX, nll_out, w.part, st));
    return LOCO_OK;
}

int loco_lm_forward(loco_lm* lm, const int32_t* tokens, const int32_t* starts, const int32_t* lens, int32_t B, int32_t S, float* const* hidden_states,
                    float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "loco_lm_forward";
    if (const int rc = check_shape(lm, fn, B, S)) return rc;
    if (!tokens || !starts || !lens || !workspace) return api_fail(LOCO_E_INVALID, "%s: null argument", fn);
    if ((long)B * S * lm->ldv > 0x7fffffffL) return api_fail(LOCO_E_INVALID, "%s: B * S * ldv exceeds 2^31 - 1 logits: this entry point is for small calls", fn);
    const LmWorkspace w = carve(lm, workspace, B, S, 0);
    if (workspace_bytes < w.bytes) return api_fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = lm_body(lm, tokens, starts, lens, B, S, w, hidden_states, st)) return rc;
    const int M = B * S;
    float* last = hidden_states ? hidden_states[lm->n_layer] : nullptr;
    if (!last && !logits) return LOCO_OK;
    HIP_TRY(launch_layernorm(w.x, lm->lnf_w, lm->lnf_b, w.ln, M, kHidden, 1e-5f, st));
    if (last) HIP_TRY(hipMemcpyAsync(last, w.ln, (size_t)M * kHidden * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (logits) {
        GemmArgs a{w.ln, lm->wte, nullptr, nullptr, logits, M, lm->ldv, kHidden, kHidden, kHidden, lm->ldv, 0, 1, 1, 0, 0, 0, 0, kEpiNone};
        HIP_TRY(launch_gemm(a, st));
    }
    return LOCO_OK;
}

size_t loco_lm_head_scratch_bytes(int64_t R, int32_t V) { return lm_head_scratch_bytes((long)R, V); }

int loco_op_lm_head_nll(const float* h, int64_t ldh, const float* wte, int64_t ldw, const int32_t* targets, int64_t R, int32_t V, int32_t ignore_index,
                        float* nll, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "loco_op_lm_head_nll";
    if (!h || !wte || !targets || !nll || !scratch) return api_fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (R < 1 || R > 0x7fffffffL || V < 1) return api_fail(LOCO_E_INVALID, "%s: R = %lld, V = %d must be >= 1", fn, (long long)R, V);
    if (ldh < kHidden || ldw < kHidden || ((ldh | ldw) & 3)) return api_fail(LOCO_E_INVALID, "%s: row strides must be >= 768 floats and multiples of 4", fn);
    if (scratch_bytes < lm_head_scratch_bytes((long)R, V))
        return api_fail(LOCO_E_WORKSPACE, "%s: scratch %zu < %zu bytes", fn, scratch_bytes, lm_head_scratch_bytes((long)R, V));
    HIP_TRY(launch_lm_head_nll(h, (long)ldh, wte, (long)ldw, targets, (long)R, V, ignore_index, nll, scratch, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_lm_embed(const int32_t* tokens, const int32_t* starts, const int32_t* lens, const float* wte, int32_t V, const float* wpe, float* x,
                     int32_t B, int32_t S, int32_t* status, void* stream) {
    const char* fn = "loco_op_lm_embed";
    if (!tokens || !starts || !lens || !wte || !wpe || !x) return api_fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (B < 1 || B > 65535 || S < 1 || V < 1) return api_fail(LOCO_E_INVALID, "%s: B = %d (1 .. 65535), S = %d, V = %d must be >= 1", fn, B, S, V);
    HIP_TRY(launch_lm_embed(tokens, starts, lens, wte, V, wpe, x, B, S, status, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_lm_group_mean(const float* nll, const int32_t* offsets, int32_t G, double* mean, double* ppl, void* stream) {
    if (!nll || !offsets || !mean || !ppl || G < 1) return api_fail(LOCO_E_INVALID, "loco_op_lm_group_mean: null argument or G < 1");
    HIP_TRY(launch_lm_group_mean(nll, offsets, G, mean, ppl, (hipStream_t)stream));
    return LOCO_OK;
}

}  // extern "C"
