// A backoff n-gram language model over the decoder's own ids, looked up on the device (include/loco_asr.h states the rule; the host
// side -- the table's construction and the entry points -- is ngram_api.hip).
//   ngram_logprobs_kernel  one wave per row: the row's last order - 1 symbols, then log P(v | them) for every v, lanes over v
//   ngram_score_kernel     one workgroup per sequence, a thread per token: log P(token i | tokens before it)
// Both resolve a candidate through ngram_chain, the one definition of the backoff chain:
//   acc = 0; for j = m .. 0: ctx = the last j symbols; if gram (ctx, w) exists return acc + logp; if j > 0 and gram ctx exists acc += bo
// in double, in that order.  The table is an open-addressing hash in HBM (loco_kernels.h, NgramTable); a lookup is a chain of dependent
// loads, so a candidate's first probes at every j are issued together before any is looked at, and the backoff weights of a row's
// contexts -- the same for every candidate -- are looked up once, lane j taking the context of j symbols.
// No atomics; nothing allocates, synchronises or depends on the host.  A row's output depends on the row's tokens and the table alone.
// Bounds: a slot index is masked into the table, a probe sequence ends after max_probe slots, a token index is below the row's count,
// a symbol outside 0 .. V makes the result NaN and is never packed into a key.
#include "loco_kernels.h"

namespace loco {

namespace {

constexpr uint32_t kNgramNone = 0xffffffffu;

__device__ __forceinline__ double ngram_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the slot that holds `key`, kNgramNone if the table has none; `first` = keys[at], already loaded
__device__ __forceinline__ uint32_t ngram_resolve(const NgramTable& t, uint64_t key, uint32_t at, uint64_t first) {
    uint64_t got = first;
    for (int i = 1; got != key && got != 0 && i < t.max_probe; ++i) {
        at = (at + 1) & t.mask;
        got = t.keys[at];
    }
    return got == key ? at : kNgramNone;
}

__device__ __forceinline__ uint32_t ngram_find(const NgramTable& t, uint64_t key) {
    const uint32_t at = (uint32_t)ngram_mix(key) & t.mask;
    return ngram_resolve(t, key, at, t.keys[at]);
}

// the last j of the m symbols packed in H (the oldest in the lowest bits)
__device__ __forceinline__ uint64_t ngram_tail(uint64_t H, int m, int j) { return (H >> (7 * (m - j))) & ((1ull << (7 * j)) - 1); }

// H = the last m = min(order - 1, n) symbols of a row of n tokens (index 0 is <s> = V); false: a token outside 0 .. V - 1
__device__ __forceinline__ bool ngram_history(const NgramTable& t, const int32_t* __restrict__ row, int n, uint64_t& H, int& m) {
    m = min(t.order - 1, n);
    H = 0;
    bool ok = true;
    for (int i = 0; i < m; ++i) {
        const int p = n - m + i;
        const int sym = p == 0 ? t.V : row[p];
        ok = ok && sym >= 0 && sym <= t.V && (p == 0 || sym < t.V);
        H |= (uint64_t)(sym & 127) << (7 * i);
    }
    return ok;
}

// the context of the last j symbols as a gram: exists, and its backoff weight
__device__ __forceinline__ bool ngram_backoff(const NgramTable& t, uint64_t H, int m, int j, double& bo) {
    const uint32_t at = ngram_find(t, ngram_key(ngram_tail(H, m, j), j));
    bo = at != kNgramNone ? t.vals[2 * (size_t)at + 1] : 0.0;
    return at != kNgramNone;
}

// bonus = weight * lp + token_bonus as a product and a sum, two roundings.  hipcc's default -ffp-contract=fast lets the backend fuse
// them into one v_fma_f64 whatever the source says: this ROCm's __dmul_rn / __dadd_rn are plain * and +, and a contract(off) pragma
// does not reach the backend's fusion.  The empty asm makes the product a value the compiler cannot look through, under any flags;
// `make` output is checked for v_mul_f64 + v_add_f64 in tests/test_ngram_ref.py.
__device__ __forceinline__ double ngram_fuse(double weight, double lp, double token_bonus) {
    double scaled = weight * lp;
    asm volatile("" : "+v"(scaled));
    return scaled + token_bonus;
}

// log P(w | H) by the chain; bo[j] / bit j of has: the context of j symbols (1 <= j <= m) and whether it exists
__device__ __forceinline__ double ngram_chain(const NgramTable& t, uint64_t H, int m, const double (&bo)[kNgramMaxOrder], unsigned has, int w) {
    uint64_t key[kNgramMaxOrder], first[kNgramMaxOrder];
    uint32_t at[kNgramMaxOrder];
#pragma unroll
    for (int j = 0; j < kNgramMaxOrder; ++j) {  // every order's first probe, independent loads
        key[j] = ngram_key(ngram_tail(H, m, min(j, m)) | ((uint64_t)w << (7 * min(j, m))), min(j, m) + 1);
        at[j] = (uint32_t)ngram_mix(key[j]) & t.mask;
        first[j] = j <= m ? t.keys[at[j]] : 0;
    }
    int jstar = -1;
    uint32_t slot = kNgramNone;
#pragma unroll
    for (int j = kNgramMaxOrder - 1; j >= 0; --j) {  // the longest gram that exists
        if (j <= m && jstar < 0) {
            const uint32_t f = ngram_resolve(t, key[j], at[j], first[j]);
            if (f != kNgramNone) jstar = j, slot = f;
        }
    }
    if (jstar < 0) return ngram_nan();  // no unigram: not a table loco_ngram_create made
    double acc = 0.0;
#pragma unroll
    for (int j = kNgramMaxOrder - 1; j >= 1; --j)
        if (j <= m && j > jstar && (has >> j & 1)) acc = __dadd_rn(acc, bo[j]);
    return __dadd_rn(acc, t.vals[2 * (size_t)slot]);
}

template <bool FUSE>
__global__ __launch_bounds__(64) void ngram_logprobs_kernel(NgramTable t, const int32_t* __restrict__ tokens, long ld, int S,
                                                            const int32_t* __restrict__ cur, int cur_offset, int R, double weight, double token_bonus,
                                                            double* __restrict__ out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= R) return;
    const int n = cur[r] + cur_offset;
    double* o = out + (long)r * t.V;
    uint64_t H = 0;
    int m = 0;
    const bool held = n >= 1 && n <= S;
    if (!held && FUSE) return;
    if (!held || !ngram_history(t, tokens + (long)r * ld, n, H, m)) {
        for (int v = lane; v < t.V; v += 64) o[v] = ngram_nan();
        return;
    }
    // lane j looks the context of j symbols up; every lane then holds all of them
    double mine = 0.0;
    bool exists = false;
    if (lane >= 1 && lane <= m) exists = ngram_backoff(t, H, m, lane, mine);
    double bo[kNgramMaxOrder];
    unsigned has = 0;
#pragma unroll
    for (int j = 1; j < kNgramMaxOrder; ++j) {
        bo[j] = __shfl(mine, j, 64);
        has |= (unsigned)(__shfl((int)exists, j, 64) != 0) << j;
    }
    bo[0] = 0.0;
    for (int v = lane; v < t.V; v += 64) {
        const double lp = ngram_chain(t, H, m, bo, has, v);
        o[v] = FUSE ? ngram_fuse(weight, lp, token_bonus) : lp;
    }
}

__global__ __launch_bounds__(256) void ngram_score_kernel(NgramTable t, const int32_t* __restrict__ tokens, const int64_t* __restrict__ starts,
                                                          const int32_t* __restrict__ lens, int64_t total, double* __restrict__ out) {
    const int b = blockIdx.x;
    const int64_t s0 = starts[b];
    const int len = lens[b];
    if (s0 < 0 || len < 0 || s0 + len > total) return;  // a sequence that leaves the buffer is not touched
    const int32_t* row = tokens + s0;
    for (int i = threadIdx.x; i < len; i += 256) {
        if (i == 0) {
            out[s0] = 0.0;
            continue;
        }
        uint64_t H = 0;
        int m = 0;
        const int w = row[i];
        if (!ngram_history(t, row, i, H, m) || w < 0 || w >= t.V) {
            out[s0 + i] = ngram_nan();
            continue;
        }
        double bo[kNgramMaxOrder];
        unsigned has = 0;
        bo[0] = 0.0;
#pragma unroll
        for (int j = 1; j < kNgramMaxOrder; ++j) {
            bo[j] = 0.0;
            if (j <= m && ngram_backoff(t, H, m, j, bo[j])) has |= 1u << j;
        }
        out[s0 + i] = ngram_chain(t, H, m, bo, has, w);
    }
}

bool ngram_table_ok(const NgramTable& t) {
    return t.keys && t.vals && t.V >= 1 && t.V <= kNgramMaxVocab && t.order >= 1 && t.order <= kNgramMaxOrder && t.max_probe >= 1 &&
           (t.mask & (t.mask + 1)) == 0;
}

}  // namespace

hipError_t launch_ngram_logprobs(const NgramTable& t, const int32_t* tokens, long ld, int S, const int32_t* cur, int cur_offset, int R, bool fuse,
                                 double weight, double token_bonus, double* out, hipStream_t s) {
    if (!ngram_table_ok(t) || !tokens || !cur || !out || R < 1 || S < 1 || ld < S) return hipErrorInvalidValue;
    if (fuse)
        hipLaunchKernelGGL(ngram_logprobs_kernel<true>, dim3(R), dim3(64), 0, s, t, tokens, ld, S, cur, cur_offset, R, weight, token_bonus, out);
    else
        hipLaunchKernelGGL(ngram_logprobs_kernel<false>, dim3(R), dim3(64), 0, s, t, tokens, ld, S, cur, cur_offset, R, weight, token_bonus, out);
    return hipGetLastError();
}

hipError_t launch_ngram_score(const NgramTable& t, const int32_t* tokens, const int64_t* starts, const int32_t* lens, int B, int64_t total,
                              double* out, hipStream_t s) {
    if (!ngram_table_ok(t) || !tokens || !starts || !lens || !out || B < 1 || total < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ngram_score_kernel, dim3(B), dim3(256), 0, s, t, tokens, starts, lens, total, out);
    return hipGetLastError();
}

}  // namespace loco
