// The rules of the text decoder that several kernels must apply alike, bit for bit (decoder.hip, decoder_pool.hip, decoder_score.hip,
// decoder_probs.hip), each written once: the argmax (generate, generate_many and score(targets = null) pick the same token), the
// attention's score and softmax tile (the probabilities are those of the attention) and the prenet's position rule (the token ids:
// loco_kernels.h).  A kernel keeps its own schedule (which thread sees which element, in what order) and its initial values.
#pragma once
#include "loco_kernels.h"

namespace loco {

constexpr int kDecPadPosition = kDecPadToken;  // the sinusoid table's zero row: HF's padding_idx, which it sets to pad_token_id
// ---- argmax ----------------------------------------------------------------------------------------------------------------
// a beats b: the first NaN wins, as in torch.argmax; otherwise the larger value, the lower index on a tie
__device__ __forceinline__ bool argmax_better(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || ai < bi);
    return av > bv || (av == bv && ai < bi);
}

// The winner among the 64 lanes' (value, index) pairs, left in every lane.  The rule is a total order on pairs of distinct indices;
// lanes that hold the same pair (the pool's lanes beyond a short row) tie and neither beats the other.
__device__ __forceinline__ void wave_argmax(float& bv, int& bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        const bool take = argmax_better(ov, oi, bv, bi);
        bv = take ? ov : bv, bi = take ? oi : bi;  // two selects: an `if` here compiles to branches
    }
}

// ---- log-softmax of a row ---------------------------------------------------------------------------------------------------
// log_softmax(x)[n] = (x[n] - mx) - logf(sum), mx the row's maximum (fmaxf over the lanes' columns, wave_max) and sum the row's
// exponentials: lane l adds columns l, l + 64, ... in that order, the lanes meet in wave_sum.  All 64 lanes of the wave must call.
__device__ __forceinline__ float row_exp_sum(const float* __restrict__ x, int V, int lane, float mx) {
    float sum = 0.f;
    for (int n = lane; n < V; n += 64) sum += expf(x[n] - mx);
    return wave_sum(sum);
}
__device__ __forceinline__ float row_logprob(float xn, float mx, float sum) { return (xn - mx) - logf(sum); }

// ---- attention -------------------------------------------------------------------------------------------------------------
struct DecAttnRow { int i, h, b; };  // query, head, clip of row = (b * kHeads + h) * Sq + i
__device__ __forceinline__ DecAttnRow dec_attn_row(long row, int Sq) {
    return {(int)(row % Sq), (int)((row / Sq) % kHeads), (int)(row / ((long)Sq * kHeads))};
}

// keys 0 .. n - 1 are visible to query i of clip b: j < kcount[b] (null: Tk) and, when causal, j <= i + causal_offset; n <= 0 (a
// negative kcount[b] included): none, the callers' loops and `j < n` tests never pass, so n is not clamped
__device__ __forceinline__ int dec_visible_keys(const int32_t* kcount, int b, int Tk, int causal, int i, int causal_offset) {
    const int nvis = kcount ? min(kcount[b], Tk) : Tk;
    return causal ? min(nvis, i + causal_offset + 1) : nvis;
}

// The three pieces below are macros, not functions: expanded as text they compile as if spelled out in place, which keeps
// dec_attention_kernel, launched 24 times per decode step, the code of profiles/decoder_rules_refactor_isa.txt; an inline function
// is unrolled before it is inlined, and the compiler then schedules and allocates that kernel differently.
// f32x4 q[16] = the head's query row at qp, times the scale, in registers
#define LOCO_DEC_LOAD_Q(q, qp, scale) \
    f32x4 q[kHeadDim / 4];            \
    _Pragma("unroll") for (int d_ = 0; d_ < kHeadDim / 4; ++d_) q[d_] = *reinterpret_cast<const f32x4*>((qp) + 4 * d_) * (scale)
// sc = q . k_j for the key row at kr: four interleaved partial sums of 16 products, combined as (a0 + a1) + (a2 + a3)
#define LOCO_DEC_QK(sc, q, kr)                                                           \
    do {                                                                                 \
        float acc_[4] = {0.f, 0.f, 0.f, 0.f};                                            \
        _Pragma("unroll") for (int d_ = 0; d_ < kHeadDim / 4; ++d_) {                    \
            const f32x4 kv_ = *reinterpret_cast<const f32x4*>((kr) + 4 * d_);            \
            acc_[0] = fmaf(q[d_].x, kv_.x, acc_[0]);                                     \
            acc_[1] = fmaf(q[d_].y, kv_.y, acc_[1]);                                     \
            acc_[2] = fmaf(q[d_].z, kv_.z, acc_[2]);                                     \
            acc_[3] = fmaf(q[d_].w, kv_.w, acc_[3]);                                     \
        }                                                                                \
        sc = (acc_[0] + acc_[1]) + (acc_[2] + acc_[3]);                                  \
    } while (0)
// One tile of 64 keys of the online softmax: sc = this lane's score (-inf and valid = false without a key; lane 0 of every tile has
// one).  Declares m_new = the new maximum, p = exp(sc - m_new) and corr = the factor for the sums kept so far (exp(-inf) = 0 on the
// first tile) and brings s_run up to date; the caller ends the tile with m_run = m_new.
#define LOCO_DEC_SOFTMAX_TILE(sc, valid, m_run, s_run, m_new, p, corr) \
    const float m_new = fmaxf(m_run, wave_max(sc));                    \
    const float p = (valid) ? expf(sc - m_new) : 0.f;                  \
    const float corr = expf(m_run - m_new);                            \
    s_run = s_run * corr + wave_sum(p)

// ---- prenet ----------------------------------------------------------------------------------------------------------------
// Row of the sinusoid table: token = (the id != kDecPadToken), the test the callers count by; cnt = non-pad tokens of the sequence up
// to and including this one; <pad> takes the zero row, padding_idx
__device__ __forceinline__ int dec_position(bool token, int cnt, int table_rows) { return min(token ? cnt + 1 : kDecPadPosition, table_rows - 1); }

// dst[0 .. 768) = embed[raw, clamped into the vocabulary] + table[dec_position], by a workgroup of 256 threads; returns the position
__device__ __forceinline__ int dec_embed_row(int raw, bool token, int cnt, const float* __restrict__ embed, int vocab, const float* __restrict__ table,
                                             int table_rows, float* __restrict__ dst) {
    const int id = min(max(raw, 0), vocab - 1);
    const int pos = dec_position(token, cnt, table_rows);
    for (int c = threadIdx.x; c < kHidden; c += 256) dst[c] = embed[(long)id * kHidden + c] + table[(long)pos * kHidden + c];
    return pos;
}

}  // namespace loco
