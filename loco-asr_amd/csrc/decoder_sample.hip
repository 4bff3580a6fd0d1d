// Sampling in the text decoder (include/loco_asr.h, loco_op_sample_tokens and loco_decoder_pool_*_sample*): temperature, top-k and
// top-p filtering and one draw per row of logits, on the device.
//   sample_tokens_kernel       the rule alone on M rows (the operator the tests drive)
//   pool_admit_samples_kernel  pool_admit_kernel for clips x copies slots, plus every slot's (utterance, hypothesis)
//   pool_sample_select_kernel  pool_select_kernel with sample_row in the argmax's place for the slots that sample
// The rule is sample_row, written once; a greedy row is the argmax of decoder_common.h, as in pool_select_kernel.
// One wave per row, lanes over columns l, l + 64, ...; no atomics; any V >= 1.  A row's token is a pure function of its V logits, the
// rule's four numbers and the row's (utterance, hypothesis, t), bit for bit: every sum is taken in an order fixed by V alone (the
// column loops run 0 .. V - 1 in every lane; the draw's prefix sums are one fixed scan over chunks of 64 columns), and the uniform is
// a counter-based Philox block that no launch, slot or neighbour feeds.  The terms are fp32 (expf); they are added in double, so a
// mass or a prefix carries the terms' own rounding and nothing that grows with V.
// The rank count of top-k and the cumulative mass of top-p are O(V) per column, O(V^2 / 64) per lane, with one division (and for
// top-p one expf) per term: for the model's V = 81 that is two columns x 81 terms per lane and pass.  That is accepted: the select
// kernel follows a step of 60-odd launches that stream the decoder's weights.  The passes are skipped when top_k is 0 or >= V and
// when top_p is 1.
#include <climits>

#include "decoder_common.h"

namespace loco {

namespace {

// Philox4x32-10 (Salmon et al., SC'11; Random123): word 0 of the block for counter c and key k
__device__ __forceinline__ uint32_t philox4x32_10_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// Inclusive prefix sums of the 64 lanes' w in lane order: a fixed scan, the same additions whatever the values
__device__ __forceinline__ double wave_scan(double w, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(w, off, 64);
        w = lane >= off ? w + o : w;
    }
    return w;
}

// The token of one row, left in every lane of the wave that calls it (all 64 lanes must).  keep (optional) [V]: 1 for the columns the
// draw ran over; for a greedy or degenerate row the argmax alone.  uniform (optional) [1]: the row's u, drawn or not.
__device__ int sample_row(const float* __restrict__ l, int V, const SampleRule& c, uint32_t utterance, uint32_t hypothesis, uint32_t t, bool greedy,
                          int32_t* __restrict__ keep, float* __restrict__ uniform) {
    const int lane = threadIdx.x & 63;
    const float T = c.temperature;
    // (1) z = l / T, an IEEE division; the argmax is that of the raw row
    float bv = -INFINITY, m = -INFINITY;
    int bi = INT_MAX;  // a lane without a column loses to every real entry (token_logprob_kernel)
    bool nan = false;
    for (int n = lane; n < V; n += 64) {
        const float v = l[n], z = __fdiv_rn(v, T);
        if (argmax_better(v, n, bv, bi)) bv = v, bi = n;
        m = fmaxf(m, z);
        nan |= z != z;
    }
    wave_argmax(bv, bi);
    m = wave_max(m);
    // (4) u = (x0 >> 8) 2^-24 in [0, 1)
    const float u = (float)(philox4x32_10_x0(utterance, hypothesis, t, 0u, c.key0, c.key1) >> 8) * 0x1p-24f;
    if (uniform && lane == 0) uniform[0] = u;
    // (6) a NaN, a +inf maximum or a row of -inf: the argmax
    bool plain = greedy || __ballot(nan) != 0ull || !(m > -INFINITY && m < INFINITY);
    float theta = INFINITY;  // column n is kept iff z_n >= theta or n is the argmax
    int token = bi;
    if (!plain) {
        // (2) top-k: n survives iff fewer than k columns lie above it; the survivors are the columns with z >= th_k
        float th_k = -INFINITY;
        if (c.top_k > 0 && c.top_k < V) {
            float mn = INFINITY;
            for (int n = lane; n < V; n += 64) {
                const float z = __fdiv_rn(l[n], T);
                int above = 0;
                for (int j = 0; j < V; ++j) above += __fdiv_rn(l[j], T) > z;
                if (above < c.top_k) mn = fminf(mn, z);
            }
            th_k = wave_min(mn);
        }
        // (3) top-p over the survivors: A_n = (sum of exp(z_j - m) over survivors with z_j <= z_n) / (the sum over all survivors),
        // both added in ascending j; kept iff A_n > 1 - top_p.  A larger z adds more non-negative terms in the same order, so the
        // kept columns are again those above a threshold, and equal logits are kept or dropped together.
        theta = th_k;
        if (c.top_p < 1.f) {
            double all = 0.0;
            for (int j = 0; j < V; ++j) {
                const float zj = __fdiv_rn(l[j], T);
                if (zj >= th_k) all += (double)expf(zj - m);
            }
            const double bar = 1.0 - (double)c.top_p;
            float mn = INFINITY;
            for (int n = lane; n < V; n += 64) {
                const float z = __fdiv_rn(l[n], T);
                if (!(z >= th_k)) continue;
                double acc = 0.0;
                for (int j = 0; j < V; ++j) {
                    const float zj = __fdiv_rn(l[j], T);
                    if (zj >= th_k && zj <= z) acc += (double)expf(zj - m);
                }
                if (acc / all > bar) mn = fminf(mn, z);
            }
            theta = wave_min(mn);
        }
        // (5) the draw: prefix sums of w over the kept columns in ascending index, chunk by chunk; Z is the last prefix
        double Z = 0.0;
        for (int base = 0; base < V; base += 64) {
            const int n = base + lane;
            double w = 0.0;
            if (n < V) {
                const float z = __fdiv_rn(l[n], T);
                if (z >= theta || n == bi) w = (double)expf(z - m);
            }
            Z += __shfl(wave_scan(w, lane), 63, 64);
        }
        plain = !(Z > 0.0 && Z < (double)INFINITY);
        if (!plain) {
            const double cut = (double)u * Z;
            double carry = 0.0;
            int last = bi;
            bool found = false;
            for (int base = 0; base < V && !found; base += 64) {
                const int n = base + lane;
                double w = 0.0;
                bool kept = false;
                if (n < V) {
                    const float z = __fdiv_rn(l[n], T);
                    kept = z >= theta || n == bi;
                    if (kept) w = (double)expf(z - m);
                }
                const double pre = wave_scan(w, lane);
                const unsigned long long over = __ballot(kept && carry + pre > cut), any = __ballot(kept);
                if (over) token = base + __ffsll((long long)over) - 1, found = true;
                if (any) last = base + 63 - __clzll((long long)any);
                carry += __shfl(pre, 63, 64);
            }
            if (!found) token = last;  // rounding left no prefix above u Z
        }
    }
    if (keep)
        for (int n = lane; n < V; n += 64) keep[n] = plain ? n == bi : (__fdiv_rn(l[n], T) >= theta || n == bi);
    return token;
}

// 256 threads = 4 waves = 4 rows; a lane never reads a column >= V of its row
__global__ __launch_bounds__(256) void sample_tokens_kernel(const float* __restrict__ logits, long ld, int M, int V, SampleRule rule,
                                                            const uint32_t* __restrict__ counters, const int32_t* __restrict__ greedy,
                                                            int32_t* __restrict__ tokens, int32_t* __restrict__ keep, float* __restrict__ uniform) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int token = sample_row(logits + row * ld, V, rule, counters[3 * row], counters[3 * row + 1], counters[3 * row + 2], greedy && greedy[row] != 0,
                                 keep ? keep + row * V : nullptr, uniform ? uniform + row : nullptr);
    if ((threadIdx.x & 63) == 0) tokens[row] = token;
}

// pool_admit_kernel for a.n slots, slot i a hypothesis of clip i / a.copies; ids [slots, 2] = (utterance, hypothesis) of every slot
__global__ __launch_bounds__(64) void pool_admit_samples_kernel(PoolState p, PoolAdmitSamples a, const int32_t* __restrict__ frames, int start,
                                                                uint32_t* __restrict__ ids) {
    const int i = threadIdx.x;
    if (i < a.n) {
        const int r = a.slot[i];
        p.tokens[(long)r * p.S_max] = start;
        p.cur[r] = start;
        p.cnt[r] = start != kDecPadToken;
        p.pos[r] = 0;
        p.cap[r] = a.cap[i];
        p.frames[r] = min(max(frames ? frames[i / a.copies] : a.rows[i], 0), a.rows[i]);  // never beyond the rows that were projected
        p.lengths[r] = 1;
        p.status[r] = kPoolOpen;
        ids[2 * r] = a.utterance[i];
        ids[2 * r + 1] = a.hypothesis[i];
    }
    __syncthreads();
    const unsigned long long open = __ballot(i < p.slots && p.status[i] == kPoolOpen);
    if (i == 0) p.poll[0] = __popcll(open);
}

// pool_select_kernel's walk and bookkeeping; bit r of `sampled` marks the slots that draw, every other live slot takes the argmax.
// step_tokens (optional) [slots]: the token a live slot appended, ignore_index for the others.
__global__ __launch_bounds__(1024) void pool_sample_select_kernel(PoolState p, const uint32_t* __restrict__ ids, unsigned long long sampled,
                                                                  SampleRule rule, const float* __restrict__ logits, int vocab, int eos,
                                                                  int32_t* __restrict__ step_tokens, int ignore_index) {
    __shared__ int open_s[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int open = 0;
    for (int r = wave; r < p.slots; r += 16) {
        const int t = p.kv_row[r], cap = p.cap[r], cnt = p.cnt[r], status = p.status[r];
        if (t >= 0) {
            const bool draws = sampled >> r & 1ull;
            const int bi = sample_row(logits + (long)r * vocab, vocab, rule, draws ? ids[2 * r] : 0u, draws ? ids[2 * r + 1] : 0u, (uint32_t)(t + 1), !draws,
                                      nullptr, nullptr);
            const bool done = bi == eos || t + 2 >= cap || t + 2 >= p.S_max;
            if (lane == 0) {
                p.tokens[(long)r * p.S_max + t + 1] = bi;
                p.lengths[r] = t + 2;
                if (done) {
                    p.status[r] = kPoolFinished;
                } else {
                    p.pos[r] = t + 1;
                    p.cur[r] = bi;
                    p.cnt[r] = cnt + (bi != kDecPadToken);
                }
                if (step_tokens) step_tokens[r] = bi;
            }
            open += !done;
        } else {
            if (status == kPoolOpen) open += 1;  // open but outside this step's bounds: the slot waits
            if (step_tokens && lane == 0) step_tokens[r] = ignore_index;
        }
    }
    if (lane == 0) open_s[wave] = open;
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < 16; ++w) n += open_s[w];
        p.poll[0] = n;
    }
}

}  // namespace

hipError_t launch_sample_tokens(const float* logits, long ld, int M, int V, const SampleRule& rule, const uint32_t* counters, const int32_t* greedy,
                                int32_t* tokens, int32_t* keep, float* uniform, hipStream_t s) {
    if (!logits || !counters || !tokens || M < 1 || V < 1 || ld < V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_tokens_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, logits, ld, M, V, rule, counters, greedy, tokens, keep,
                       uniform);
    return hipGetLastError();
}

hipError_t launch_pool_admit_samples(const PoolState& p, const PoolAdmitSamples& a, const int32_t* frames, int start, uint32_t* ids, hipStream_t s) {
    if (p.slots <= 0 || p.slots > kSkinnyMaxM || a.n <= 0 || a.n > p.slots || a.copies < 1 || a.n % a.copies || !ids) return hipErrorInvalidValue;
    for (int i = 0; i < a.n; ++i)
        if (a.slot[i] < 0 || a.slot[i] >= p.slots || a.cap[i] < 2 || a.cap[i] > p.S_max || a.rows[i] < 1 || a.rows[i] > p.T_cap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_admit_samples_kernel, dim3(1), dim3(64), 0, s, p, a, frames, start, ids);
    return hipGetLastError();
}

hipError_t launch_pool_sample_select(const PoolState& p, const uint32_t* ids, unsigned long long sampled, const SampleRule& rule, const float* logits,
                                     int vocab, int eos, int32_t* step_tokens, int ignore_index, hipStream_t s) {
    if (p.slots <= 0 || p.slots > kSkinnyMaxM || vocab < 1 || !ids) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_sample_select_kernel, dim3(1), dim3(1024), 0, s, p, ids, sampled, rule, logits, vocab, eos, step_tokens, ignore_index);
    return hipGetLastError();
}

}  // namespace loco
