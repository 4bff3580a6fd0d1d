// Host side of the n-gram language model (include/loco_asr.h, loco_ngram_* and loco_op_ngram_*): the checks every gram passes, the
// hash table built on the host and copied to the device once, and the two scoring entry points over ngram.hip's kernels.
#include <cmath>
#include <cstring>
#include <new>

#include "loco_host.h"

using namespace loco;
using namespace loco::host;

namespace {

void ngram_free(loco_ngram* g) {
    if (!g) return;
    if (g->keys) (void)hipFree(g->keys);
    if (g->vals) (void)hipFree(g->vals);
    delete g;
}

}  // namespace

int loco_ngram_create(int32_t vocab, int32_t order, int64_t n, const int32_t* lengths, const int32_t* symbols, const double* logp,
                      const double* backoff, loco_ngram** out) {
    const char* fn = "loco_ngram_create";
    if (!out) return fail(LOCO_E_INVALID, "%s: null out", fn);
    *out = nullptr;
    if (vocab < 1 || vocab > kNgramMaxVocab) return fail(LOCO_E_INVALID, "%s: vocab = %d is outside 1 .. %d", fn, vocab, kNgramMaxVocab);
    if (order < 1 || order > kNgramMaxOrder) return fail(LOCO_E_INVALID, "%s: order = %d is outside 1 .. %d", fn, order, kNgramMaxOrder);
    if (n < 1 || n > kNgramMaxGrams) return fail(LOCO_E_INVALID, "%s: n = %lld grams is outside 1 .. 2^26", fn, (long long)n);
    if (!lengths || !symbols || !logp || !backoff) return fail(LOCO_E_INVALID, "%s: null lengths, symbols, logp or backoff", fn);
    const int V = vocab, BOS = vocab;
    uint64_t slots = 64;
    while (slots < 2 * (uint64_t)n) slots <<= 1;  // load factor <= 0.5
    const uint32_t mask = (uint32_t)(slots - 1);
    std::vector<uint64_t> keys;
    std::vector<double> vals;
    std::vector<int32_t> owner;
    try {  // 28 bytes per slot on the host: 3.5 GiB at the limit of 2^26 grams
        keys.assign(slots, 0);
        vals.assign(2 * slots, 0.0);
        owner.assign(slots, -1);
    } catch (const std::bad_alloc&) {
        return fail(LOCO_E_INVALID, "%s: no host memory to build a table of %llu slots (%llu bytes) for n = %lld grams", fn,
                    (unsigned long long)slots, (unsigned long long)(slots * 28), (long long)n);
    }
    int max_probe = 1;
    for (int64_t i = 0; i < n; ++i) {
        const int len = lengths[i];
        if (len < 1 || len > order) return fail(LOCO_E_INVALID, "%s: gram %lld has length %d, outside 1 .. order = %d", fn, (long long)i, len, order);
        uint64_t packed = 0;
        for (int p = 0; p < len; ++p) {
            const int sym = symbols[i * kNgramMaxOrder + p];
            if (sym < 0 || sym > BOS)
                return fail(LOCO_E_INVALID, "%s: gram %lld: symbol %d at position %d is outside 0 .. %d (%d = <s>)", fn, (long long)i, sym, p, BOS, BOS);
            if (sym == BOS && p == len - 1 && len > 1)
                return fail(LOCO_E_INVALID, "%s: gram %lld: <s> (%d) in the predicted position", fn, (long long)i, BOS);
            if (sym == BOS && p != 0)
                return fail(LOCO_E_INVALID, "%s: gram %lld: <s> (%d) at position %d of its context; it may open a context only", fn, (long long)i, BOS, p);
            packed |= (uint64_t)sym << (7 * p);
        }
        if (!std::isfinite(logp[i])) return fail(LOCO_E_INVALID, "%s: gram %lld: logp is not finite", fn, (long long)i);
        if (!std::isfinite(backoff[i])) return fail(LOCO_E_INVALID, "%s: gram %lld: backoff is not finite", fn, (long long)i);
        const uint64_t key = ngram_key(packed, len);
        uint32_t at = (uint32_t)ngram_mix(key) & mask;
        int probes = 1;
        while (keys[at] != 0) {
            if (keys[at] == key) return fail(LOCO_E_INVALID, "%s: gram %lld is a duplicate of gram %d", fn, (long long)i, owner[at]);
            at = (at + 1) & mask, ++probes;
        }
        keys[at] = key, owner[at] = (int32_t)i;
        vals[2 * (size_t)at] = logp[i], vals[2 * (size_t)at + 1] = backoff[i];
        max_probe = std::max(max_probe, probes);
    }
    for (int w = 0; w < V; ++w) {
        const uint64_t key = ngram_key((uint64_t)w, 1);
        uint32_t at = (uint32_t)ngram_mix(key) & mask;
        while (keys[at] != 0 && keys[at] != key) at = (at + 1) & mask;
        if (keys[at] != key) return fail(LOCO_E_INVALID, "%s: symbol %d has no unigram: every id 0 .. %d needs one", fn, w, V - 1);
    }
    loco_ngram* g = new (std::nothrow) loco_ngram();
    if (!g) return fail(LOCO_E_INVALID, "%s: no host memory for the handle", fn);
    (void)hipGetDevice(&g->device);
    g->grams = n;
    if (hipMalloc(&g->keys, slots * sizeof(uint64_t)) != hipSuccess || hipMalloc(&g->vals, 2 * slots * sizeof(double)) != hipSuccess ||
        hipMemcpy(g->keys, keys.data(), slots * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->vals, vals.data(), 2 * slots * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        ngram_free(g);
        return fail(LOCO_E_HIP, "%s: a table of %llu slots (%llu bytes) could not be placed on the device", fn, (unsigned long long)slots,
                    (unsigned long long)(slots * 24));
    }
    g->table = NgramTable{g->keys, g->vals, mask, max_probe, V, order};
    *out = g;
    return LOCO_OK;
}

void loco_ngram_destroy(loco_ngram* g) { ngram_free(g); }

int32_t loco_ngram_vocab(const loco_ngram* g) { return g ? g->table.V : 0; }

int32_t loco_ngram_order(const loco_ngram* g) { return g ? g->table.order : 0; }

int loco_op_ngram_logprobs(const loco_ngram* g, const int32_t* tokens, int64_t ld, int32_t S, const int32_t* cur, int32_t R, double* out,
                           void* stream) {
    const char* fn = "loco_op_ngram_logprobs";
    if (!g || !tokens || !cur || !out) return fail(LOCO_E_INVALID, "%s: null model, tokens, cur or out", fn);
    if (R < 1 || R > (1 << 24)) return fail(LOCO_E_INVALID, "%s: R = %d rows is outside 1 .. 2^24", fn, R);
    if (S < 1 || ld < S) return fail(LOCO_E_INVALID, "%s: S = %d must be >= 1 and the row stride ld = %lld >= S", fn, S, (long long)ld);
    HIP_TRY(launch_ngram_logprobs(g->table, tokens, (long)ld, S, cur, 0, R, false, 1.0, 0.0, out, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_ngram_score(const loco_ngram* g, const int32_t* tokens, int64_t total, const int64_t* starts, const int32_t* lens, int32_t B,
                        double* out, void* stream) {
    const char* fn = "loco_op_ngram_score";
    if (!g || !tokens || !starts || !lens || !out) return fail(LOCO_E_INVALID, "%s: null model, tokens, starts, lens or out", fn);
    if (B < 1 || B > (1 << 24)) return fail(LOCO_E_INVALID, "%s: B = %d sequences is outside 1 .. 2^24", fn, B);
    if (total < 0) return fail(LOCO_E_INVALID, "%s: total = %lld tokens", fn, (long long)total);
    HIP_TRY(launch_ngram_score(g->table, tokens, starts, lens, B, total, out, (hipStream_t)stream));
    return LOCO_OK;
}
