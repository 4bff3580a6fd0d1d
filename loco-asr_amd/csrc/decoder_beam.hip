// Beam search in the decoder slot pool (include/loco_asr.h, loco_op_beam_* and loco_decoder_pool_*_beam*): the selection rule, the
// finished-hypothesis lists and the reordering of a group's rows by parent beam, on the device.
//   pool_admit_beams_kernel  pool_admit_kernel for groups of K slots: beam 0 alive with score 0, the list empty
//   beam_select_kernel       one wave per group: log-softmax of the K rows, the 2K best candidates, the list, the next beams
//                            (<true>: with a per-candidate bonus, the n-gram fusion; ngram.hip computes it)
//   beam_poll_kernel         poll[0] = slots open (the select kernel's groups run in separate workgroups)
//   beam_copy_kernel         rows 0 .. count - 1 of a slot from its parent's into the shadow, then from the shadow back
// The rule is HF's _beam_search with flags in place of its -1e9 sentinels and scores carried in double (include/loco_asr.h states it).
// A candidate is (score, flat index k V + v); beam_before is a total order on candidates of distinct indices, so the 2K best and
// their order depend on the values alone: round j takes the best candidate that comes after round j - 1's, every lane scanning its
// own columns and the lanes meeting in a butterfly.  That is O(2K K V / 64) per lane, two columns x K rows x 2K rounds for the
// model's V = 81; the kernel follows a step of 60-odd launches that stream the decoder's weights.
// A row's log-probabilities are decoder_common.h's (token_logprob_kernel's arithmetic); the kernel writes them out and reads the
// candidates from what it wrote.  No atomics; nothing allocates, synchronises or depends on the host.
// Bounds: a group runs only if its first slot is open and the step wrote a cache row for it; the position is below S_max - 1, the
// list's count is clamped to K, the den index into its table, a parent into its own group.
#include <climits>

#include "decoder_common.h"

namespace loco {

namespace {

constexpr long kBeamCopyChunk = 12288;  // 4-byte words one workgroup copies: 8 cache rows of k|v

// a comes before b: the larger score, the lower index on a tie; a NaN after every number, NaNs among themselves by index
__device__ __forceinline__ bool beam_before(double as, int ai, double bs, int bi) {
    const bool an = as != as, bn = bs != bs;
    if (an || bn) return (an && bn) ? ai < bi : bn;
    return as > bs || (as == bs && ai < bi);
}

// a finished score a ranks strictly above b (the list's stable insertion): a number above every NaN, NaNs equal
__device__ __forceinline__ bool beam_score_above(double a, double b) { return a == a && (b != b || a > b); }

__global__ __launch_bounds__(64) void pool_admit_beams_kernel(PoolState p, BeamState b, PoolAdmitSamples a, const int32_t* __restrict__ frames,
                                                              int start) {
    const int i = threadIdx.x;
    if (i < a.n) {
        const int r = a.slot[i], k = i % a.copies;
        p.tokens[(long)r * p.S_max] = start;
        p.cur[r] = start;
        p.cnt[r] = start != kDecPadToken;
        p.pos[r] = 0;
        p.cap[r] = a.cap[i];
        p.frames[r] = min(max(frames ? frames[i / a.copies] : a.rows[i], 0), a.rows[i]);  // never beyond the rows that were projected
        p.lengths[r] = 1;
        p.status[r] = kPoolOpen;
        b.tlp[(long)r * p.S_max] = 0.f;
        b.run[r] = k == 0 ? 0.0 : -1e9;
        b.alive[r] = k == 0;
        b.parent[r] = r;
        b.count[r] = 0;
        if (k == 0) {
            const int g = r / a.copies;
            b.unsat[g] = 1;
            b.fin_n[g] = 0;
        }
    }
    __syncthreads();
    const unsigned long long open = __ballot(i < p.slots && p.status[i] == kPoolOpen);
    if (i == 0) p.poll[0] = __popcll(open);
}

// FUSED: candidate (k, v) scores (run[k] + lp[k][v]) + bonus[k][v], bonus f64 [slots, V] (the n-gram fusion of include/loco_asr.h); the
// sum is two roundings, never a contraction.  <false> never reads bonus: the rule's arithmetic as it was.
template <bool FUSED>
__global__ __launch_bounds__(64) void beam_select_kernel(PoolState p, BeamState b, BeamRule rule, const float* __restrict__ logits, long ld, int V,
                                                         int eos, float* logprobs, const double* __restrict__ bonus) {
    __shared__ double run_s[kBeamMax], cand_s[2 * kBeamMax], m_s[2 * kBeamMax];
    __shared__ int alive_s[kBeamMax], cnt_s[kBeamMax], cand_i[2 * kBeamMax], m_src[2 * kBeamMax], next_c[kBeamMax], plan[4];
    const int lane = threadIdx.x, g = blockIdx.x;
    const int K = min(max(rule.K, 1), kBeamMax), S = p.S_max;
    const int base = g * K;
    if (g >= b.groups || base + K > p.slots) return;
    if (p.status[base] != kPoolOpen) return;  // a group that is not open reads and writes nothing
    const int t = p.kv_row[base];
    if (t < 0 || t + 1 >= S) {  // open but outside this step's bounds: the group waits, and the reorder has nothing to move
        if (lane < K) b.parent[base + lane] = base + lane, b.count[base + lane] = 0;
        return;
    }
    const int cur = t + 1, cap = p.cap[base];  // cur tokens in every running beam; cur < S
    if (lane < K) {
        alive_s[lane] = b.alive[base + lane] != 0;
        run_s[lane] = b.run[base + lane];
        cnt_s[lane] = p.cnt[base + lane];
    }
    // (1) the K rows' log-softmax
    for (int k = 0; k < K; ++k) {
        const float* x = logits + (long)(base + k) * ld;
        float mx = -INFINITY;
        for (int n = lane; n < V; n += 64) mx = fmaxf(mx, x[n]);
        mx = wave_max(mx);
        const float sum = row_exp_sum(x, V, lane, mx);
        for (int n = lane; n < V; n += 64) logprobs[(long)(base + k) * V + n] = row_logprob(x[n], mx, sum);
    }
    __syncthreads();
    // (2) the 2K best candidates, in order
    int ncand = 0, last_i = -1;
    double last_s = 0.0;
    for (int j = 0; j < 2 * K; ++j) {
        double bs = 0.0;
        int bi = INT_MAX;  // no candidate yet
        for (int k = 0; k < K; ++k) {
            if (!alive_s[k]) continue;
            const float* row = logprobs + (long)(base + k) * V;
            const double rk = run_s[k];
            for (int v = lane; v < V; v += 64) {
                double s = rk + (double)row[v];
                if (FUSED) s = __dadd_rn(s, bonus[(long)(base + k) * V + v]);
                const int c = k * V + v;
                if (j > 0 && !beam_before(last_s, last_i, s, c)) continue;
                if (bi == INT_MAX || beam_before(s, c, bs, bi)) bs = s, bi = c;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double os = __shfl_xor(bs, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            const bool take = oi != INT_MAX && (bi == INT_MAX || beam_before(os, oi, bs, bi));
            bs = take ? os : bs, bi = take ? oi : bi;
        }
        if (bi == INT_MAX) break;  // fewer candidates than 2K: no beam alive (the same in every lane)
        if (lane == 0) cand_s[j] = bs, cand_i[j] = bi;
        last_s = bs, last_i = bi, ncand = j + 1;
    }
    __syncthreads();
    // (3) - (7) on one lane: the merged list (m_src: < kBeamMax an old entry, else kBeamMax + candidate), the next beams, the flags
    const bool at_cap = cur + 1 >= cap || cur + 1 >= S;
    if (lane == 0) {
        int m = min(max(b.fin_n[g], 0), K);
        bool unsat = b.unsat[g] != 0;
        const bool update = unsat && !(rule.early == 1 && m >= K);
        for (int e = 0; e < m; ++e) m_s[e] = b.fin_score[base + e], m_src[e] = e;
        const double den_cur = b.den[min(max(cur, 1), b.den_n - 1)];
        if (update)
            for (int c = 0; c < min(K, ncand); ++c) {
                if (!(cand_i[c] % V == eos || at_cap)) continue;
                const double sc = cand_s[c] / den_cur;
                int at = m;
                while (at > 0 && beam_score_above(sc, m_s[at - 1])) m_s[at] = m_s[at - 1], m_src[at] = m_src[at - 1], --at;
                m_s[at] = sc, m_src[at] = kBeamMax + c, ++m;
            }
        m = min(m, K);
        int nn = 0;
        for (int c = 0; c < ncand && nn < K; ++c)
            if (!(cand_i[c] % V == eos || at_cap)) next_c[nn++] = c;
        bool done = true;
        if (nn > 0) {
            const int L = min(max((rule.early == 2 && rule.penalty_positive) ? cap - 1 : cur, 1), b.den_n - 1);
            const double worst = m >= K ? m_s[K - 1] : -1e9;
            unsat = unsat && cand_s[next_c[0]] / b.den[L] > worst;
            done = !unsat || (rule.early == 1 && m >= K);
        }
        plan[0] = m, plan[1] = nn, plan[2] = done, plan[3] = unsat;
    }
    __syncthreads();
    const int m = plan[0], nn = plan[1], done = plan[2];
    // the list, last entry first: an old entry only ever moves down, so its target has been moved on (or dropped) before it is written
    for (int q = m - 1; q >= 0; --q) {
        const int src = m_src[q];
        const long dst = (long)(base + q) * S;
        if (src >= kBeamMax) {
            const int c = src - kBeamMax, k = cand_i[c] / V, tok = cand_i[c] % V;
            const long from = (long)(base + k) * S;
            for (int i = lane; i < cur; i += 64) b.fin_tok[dst + i] = p.tokens[from + i], b.fin_tlp[dst + i] = b.tlp[from + i];
            if (lane == 0) {
                b.fin_tok[dst + cur] = tok;
                b.fin_tlp[dst + cur] = logprobs[(long)(base + k) * V + tok];
                b.fin_score[base + q] = m_s[q];
                b.fin_sum[base + q] = cand_s[c];
                b.fin_len[base + q] = cur + 1;
            }
        } else if (src != q) {
            const long from = (long)(base + src) * S;
            const int len = b.fin_len[base + src], n = min(max(len, 0), S);
            const double sum = b.fin_sum[base + src];
            for (int i = lane; i < n; i += 64) b.fin_tok[dst + i] = b.fin_tok[from + i], b.fin_tlp[dst + i] = b.fin_tlp[from + i];
            if (lane == 0) b.fin_score[base + q] = m_s[q], b.fin_sum[base + q] = sum, b.fin_len[base + q] = len;
        }
        __syncthreads();
    }
    // the next running beams: slot base + lane takes candidate next_c[lane]; its rows 0 .. cur - 1 follow in the reorder
    if (lane < K) {
        const int r = base + lane;
        int par = lane, tok = kDecPadToken, al = 0, cnt = cnt_s[lane];
        float lp = 0.f;
        double sc = -1e9;
        if (lane < nn) {
            const int c = next_c[lane];
            par = cand_i[c] / V, tok = cand_i[c] % V, al = 1;
            lp = logprobs[(long)(base + par) * V + tok];
            sc = cand_s[c];
            cnt = cnt_s[par] + (tok != kDecPadToken);
        }
        p.tokens[(long)r * S + cur] = tok;
        b.tlp[(long)r * S + cur] = lp;
        b.run[r] = sc;
        b.alive[r] = al;
        b.parent[r] = base + par;
        b.count[r] = done ? 0 : cur;
        p.lengths[r] = cur + 1;
        if (done) {
            p.status[r] = kPoolFinished;
        } else {
            p.pos[r] = t + 1;
            p.cur[r] = tok;
            p.cnt[r] = cnt;
        }
    }
    if (lane == 0) b.unsat[g] = plan[3], b.fin_n[g] = m;
}

__global__ __launch_bounds__(64) void beam_poll_kernel(PoolState p) {
    const int i = threadIdx.x;
    const unsigned long long open = __ballot(i < p.slots && p.status[i] == kPoolOpen);
    if (i == 0) p.poll[0] = __popcll(open);
}

// dst slot r, words [0, count[r] W) := src slot (from_parent ? parent[r] : r), for the slots whose parent differs (and, with `open`,
// whose status is open); workgroup x copies one chunk.  VEC: W % 4 == 0 and both buffers 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void beam_copy_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int from_parent, int slots,
                                                        long slot_words, long W, int S, const int32_t* __restrict__ parent,
                                                        const int32_t* __restrict__ count, const int32_t* __restrict__ open, int K) {
    const int r = blockIdx.y, l = blockIdx.z;
    if (open && open[r] != kPoolOpen) return;
    const int lo = r / K * K, hi = min(lo + K - 1, slots - 1);
    const int par = min(max(parent[r], lo), hi);
    if (par == r) return;
    const long words = (long)min(max(count[r], 0), S) * W;
    const long start = (long)blockIdx.x * kBeamCopyChunk;
    if (start >= words) return;
    const long end = min(start + kBeamCopyChunk, words);
    const uint32_t* from = src + ((long)l * slots + (from_parent ? par : r)) * slot_words;
    uint32_t* to = dst + ((long)l * slots + r) * slot_words;
    if (VEC) {
        for (long i = start + 4 * (long)threadIdx.x; i < end; i += 1024) *reinterpret_cast<uint4*>(to + i) = *reinterpret_cast<const uint4*>(from + i);
    } else {
        for (long i = start + threadIdx.x; i < end; i += 256) to[i] = from[i];
    }
}

}  // namespace

hipError_t launch_pool_admit_beams(const PoolState& p, const BeamState& b, const PoolAdmitSamples& a, const int32_t* frames, int start, hipStream_t s) {
    const int K = a.copies;
    if (p.slots <= 0 || p.slots > kSkinnyMaxM || K < 1 || K > kBeamMax || a.n <= 0 || a.n > p.slots || a.n % K || b.groups != p.slots / K)
        return hipErrorInvalidValue;
    for (int i = 0; i < a.n; ++i)
        if (a.slot[i] < 0 || a.slot[i] >= b.groups * K || a.slot[i] % K != i % K || a.slot[i] - a.slot[i - i % K] != i % K || a.cap[i] < 2 ||
            a.cap[i] > p.S_max || a.rows[i] < 1 || a.rows[i] > p.T_cap)
            return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_admit_beams_kernel, dim3(1), dim3(64), 0, s, p, b, a, frames, start);
    return hipGetLastError();
}

hipError_t launch_beam_select(const PoolState& p, const BeamState& b, const BeamRule& rule, const float* logits, long ld, int V, int eos,
                              float* logprobs, hipStream_t s, const double* bonus) {
    if (p.slots <= 0 || rule.K < 1 || rule.K > kBeamMax || b.groups < 1 || (long)b.groups * rule.K > p.slots || V < 2 * rule.K || V > (1 << 20) ||
        ld < V || p.S_max < 2 || b.den_n < 2 || !logits || !logprobs || (p.poll && p.slots > 64))
        return hipErrorInvalidValue;
    if (bonus)
        hipLaunchKernelGGL(beam_select_kernel<true>, dim3(b.groups), dim3(64), 0, s, p, b, rule, logits, ld, V, eos, logprobs, bonus);
    else
        hipLaunchKernelGGL(beam_select_kernel<false>, dim3(b.groups), dim3(64), 0, s, p, b, rule, logits, ld, V, eos, logprobs, bonus);
    if (p.poll) hipLaunchKernelGGL(beam_poll_kernel, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_beam_reorder(void* buf, void* shadow, int layers, int slots, int S, long W, const int32_t* parent, const int32_t* count,
                               const int32_t* open, int K, int max_count, hipStream_t s) {
    if (!buf || !shadow || !parent || !count || layers < 1 || layers > 65535 || slots < 1 || slots > 65535 || S < 1 || W < 1 || K < 1 || max_count < 0)
        return hipErrorInvalidValue;
    const long words = (long)min(max_count, S) * W;
    if (words == 0) return hipSuccess;
    const long chunks = (words + kBeamCopyChunk - 1) / kBeamCopyChunk;
    if (chunks > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)chunks, slots, layers);
    const long slot_words = (long)S * W;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(buf) & 15) == 0 && (reinterpret_cast<uintptr_t>(shadow) & 15) == 0;
    const uint32_t* cb = static_cast<const uint32_t*>(buf);
    const uint32_t* cs = static_cast<const uint32_t*>(shadow);
    if (vec) {
        hipLaunchKernelGGL(beam_copy_kernel<true>, grid, dim3(256), 0, s, cb, static_cast<uint32_t*>(shadow), 1, slots, slot_words, W, S, parent, count, open, K);
        hipLaunchKernelGGL(beam_copy_kernel<true>, grid, dim3(256), 0, s, cs, static_cast<uint32_t*>(buf), 0, slots, slot_words, W, S, parent, count, open, K);
    } else {
        hipLaunchKernelGGL(beam_copy_kernel<false>, grid, dim3(256), 0, s, cb, static_cast<uint32_t*>(shadow), 1, slots, slot_words, W, S, parent, count, open, K);
        hipLaunchKernelGGL(beam_copy_kernel<false>, grid, dim3(256), 0, s, cs, static_cast<uint32_t*>(buf), 0, slots, slot_words, W, S, parent, count, open, K);
    }
    return hipGetLastError();
}

}  // namespace loco
