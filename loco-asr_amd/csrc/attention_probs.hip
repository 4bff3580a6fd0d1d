// Attention probabilities for output_attentions=True (HF modeling_speecht5.py:930-955): for clip b, head h, query i < T and
// every key j < T
//
//   S[i,j]      = q_scaled[i] . k[j] + qp[b,h,i, clip(i-j,-160,159)+160]
//   P[b,h,i,j]  = exp(S[i,j] - m_i) / l_i    for j < frames[b]    (m_i, l_i: max and sum over the valid keys)
//   P[b,h,i,j]  = 0                          for j >= frames[b]   (HF's additive finfo.min key mask after exp)
//
// Padded query rows (i >= frames[b]) are written like any other, as HF writes them.  This is a separate, store-bound
// kernel: the flash kernels never form P, and nothing here changes them.  It runs right after the layer's attention
// launch and reads what that launch read: q, k and the relative-position table qp.
//
// Operand forms (template F16):
//   false -- exact-fp32 mode: qkv [B,T,2304] fp32 (q pre-scaled) and the full qp [B,12,T,320] of the table GEMM, products on
//            v_mfma_f32_32x32x2_f32.
//   true  -- f16x3 / f16x2: q and k as fp16 hi/lo planes [B*T,768], products on v_mfma_f32_32x32x16_f16 (terms 3: Qlo Khi +
//            Qhi Klo + Qhi Khi; terms 2: the Klo term dropped).  qp is the scratch the f16x3 attention launch has just filled: only
//            some 32-column blocks of it are formed (include/loco_asr.h, loco_op_attention_f16x3_pe), and for a wave whose every
//            valid key is past-clipped none at all.  So a masked key is SET to 0 and never reads qp, and a query row i >= frames[b] +
//            158, whose valid keys would all read column 319, adds 0 to every score instead (both forms: one rule).
//
// What a launch reads of clip b with n = frames[b] valid keys (the contract of include/loco_asr.h): q rows [0, T); k rows [0, 32 ceil(n / 32)),
// capped at T, those from n on discarded by a select; of table row i the entries clip(i - n + 1) + 160 ... clip(i) + 160 if i < n + 158, none otherwise.
//
// Schedule: one workgroup = 4 waves = 128 consecutive query rows of one (clip, head); each wave owns 32 rows as one 32x32
// accumulator S = Q K^T per key tile, with the QUERY as the MFMA's m index and the KEY as its n index, so lane (n, half) holds
// key n of the tile and row 8 (e>>2) + 4 half + (e&3) in register e.  (Two accumulators per wave, 64 rows, took 370 registers:
// one wave per SIMD.)  The four waves walk the same K tiles at the same time and share them
// through the CU's L1.
//   pass 1: over the valid key tiles, per lane and row an online (max, sum) in the log2 domain; then one reduction over the 32
//           lanes of each half (the lanes that hold the same rows) gives m_i and l_i.
//   pass 2: the same products again (the same instruction sequence: bit-identical scores), P = exp2(S log2e - m) / l, and the
//           store straight from the accumulator: one register is two 128-byte row segments per wave instruction (lanes 0-31:
//           row i, keys j0..j0+31; lanes 32-63: row i+4), the full-rate store shape.  Key tiles past frames[b] are written as
//           zeros without any arithmetic.
// Offsets into P are 64-bit: one layer of P passes 2^31 elements from T ~ 13 400 at B = 1.
#include "loco_kernels.h"

namespace loco {

typedef _Float16 ap_h8 __attribute__((ext_vector_type(8)));

constexpr int AP_NST = 1;                   // 32-row accumulators per wave
constexpr int AP_WROWS = 32 * AP_NST;       // query rows per wave
constexpr int AP_BQ = 4 * AP_WROWS;         // per workgroup
constexpr int AP_BK = 32;                   // keys per tile

template <bool F16>
__global__ __launch_bounds__(256) void attention_probs_kernel(const float* __restrict__ qkv, const _Float16* __restrict__ qhi,
                                                              const _Float16* __restrict__ qlo, const _Float16* __restrict__ khi,
                                                              const _Float16* __restrict__ klo, const float* __restrict__ qp,
                                                              const int32_t* __restrict__ frames, float* __restrict__ probs, int T,
                                                              int nqb, int terms) {
    const int qblk = blockIdx.x % nqb;
    const int head = (blockIdx.x / nqb) % kHeads;
    const int b = blockIdx.x / (nqb * kHeads);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int i0 = qblk * AP_BQ + wave * AP_WROWS;  // first query row of this wave
    if (i0 >= T) return;                            // no barrier below: a wave past the end simply leaves

    int nvalid = frames ? frames[b] : T;
    if (nvalid <= 0 || nvalid > T) nvalid = T;  // as the attention kernels
    const int ntv = (nvalid + AP_BK - 1) / AP_BK;  // key tiles holding a valid key
    const int nt = (T + AP_BK - 1) / AP_BK;
    constexpr float kLog2e = 1.4426950408889634f;

    // ---- Q fragments (A operand): F32 -- q[st][kk] = Q[i0 + 32 st + r][32 h + kk];  F16 -- step ks: Q[..][16 ks + 8 h + 0..7]
    float qf[F16 ? 1 : AP_NST][32];
    ap_h8 qfh[F16 ? AP_NST : 1][4], qfl[F16 ? AP_NST : 1][4];
#pragma unroll
    for (int st = 0; st < AP_NST; ++st) {
        int i = i0 + 32 * st + r;
        i = i < T ? i : T - 1;
        if constexpr (F16) {
            const long o = ((long)b * T + i) * kHidden + head * kHeadDim + 8 * h;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                qfh[st][ks] = *reinterpret_cast<const ap_h8*>(qhi + o + 16 * ks);
                qfl[st][ks] = *reinterpret_cast<const ap_h8*>(qlo + o + 16 * ks);
            }
        } else {
            const f32x4* p = reinterpret_cast<const f32x4*>(qkv + ((long)b * T + i) * kQkv + head * kHeadDim + 32 * h);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const f32x4 v = p[c];
#pragma unroll
                for (int e = 0; e < 4; ++e) qf[st][4 * c + e] = v[e];
            }
        }
    }
    const float* qpb = qp + ((long)b * kHeads + head) * T * kRelN;

    // S (the 32-row accumulators) of key tile t, relative-position bias added for the valid keys; log2 domain
    f32x16 acc[AP_NST];
    auto scores = [&](int t) {
        const int j0 = t * AP_BK;
        int jk = j0 + r;
        jk = jk < T ? jk : T - 1;
#pragma unroll
        for (int st = 0; st < AP_NST; ++st)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[st][e] = 0.f;
        if constexpr (F16) {
            const long o = ((long)b * T + jk) * kHidden + head * kHeadDim + 8 * h;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const ap_h8 kh = *reinterpret_cast<const ap_h8*>(khi + o + 16 * ks);
                const ap_h8 kl = *reinterpret_cast<const ap_h8*>(klo + o + 16 * ks);
#pragma unroll
                for (int st = 0; st < AP_NST; ++st) {
                    acc[st] = __builtin_amdgcn_mfma_f32_32x32x16_f16(qfl[st][ks], kh, acc[st], 0, 0, 0);
                    if (terms > 2) acc[st] = __builtin_amdgcn_mfma_f32_32x32x16_f16(qfh[st][ks], kl, acc[st], 0, 0, 0);
                    acc[st] = __builtin_amdgcn_mfma_f32_32x32x16_f16(qfh[st][ks], kh, acc[st], 0, 0, 0);
                }
            }
        } else {
            const f32x4* p = reinterpret_cast<const f32x4*>(qkv + ((long)b * T + jk) * kQkv + kHidden + head * kHeadDim + 32 * h);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const f32x4 kv = p[c];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int st = 0; st < AP_NST; ++st)
                        acc[st] = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[st][4 * c + e], kv[e], acc[st], 0, 0, 0);
            }
        }
        const int j = j0 + r;
        if (j < nvalid) {  // masked keys never read the table (its entries there may be stale scratch)
#pragma unroll
            for (int st = 0; st < AP_NST; ++st)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    int i = i0 + 32 * st + 8 * (e >> 2) + 4 * h + (e & 3);
                    i = i < T ? i : T - 1;
                    // a row whose every valid key is past-clipped (its nearest one, nvalid - 1, included) would add column 319 to all of
                    // them: a bias that is constant over the row cancels in the softmax, so the row adds 0 and reads no entry.  The f16x3
                    // attention launch forms NO block for a wave of such rows (its c_past is 0 as well): their scratch is unformed
                    float bias = 0.f;
                    if (i - (nvalid - 1) < kRelMax - 1) {
                        int rel = i - j;
                        rel = rel < -kRelMax ? -kRelMax : (rel > kRelMax - 1 ? kRelMax - 1 : rel);
                        bias = qpb[(long)i * kRelN + rel + kRelMax];
                    }
                    acc[st][e] = (acc[st][e] + bias) * kLog2e;
                }
        }
        // the score is rounded here, in both passes: without the barrier the compiler contracts it into the next operation
        // differently at the two call sites, and pass 2 then exponentiates a score pass 1 never saw (a one-key row gives 1 - 1 ulp)
#pragma unroll
        for (int st = 0; st < AP_NST; ++st)
#pragma unroll
            for (int e = 0; e < 16; ++e) asm volatile("" : "+v"(acc[st][e]));
    };

    // ---- pass 1: per lane and row, online max / sum over this lane's valid keys
    float m[AP_NST][16], l[AP_NST][16];
#pragma unroll
    for (int st = 0; st < AP_NST; ++st)
#pragma unroll
        for (int e = 0; e < 16; ++e) { m[st][e] = -INFINITY; l[st][e] = 0.f; }
    for (int t = 0; t < ntv; ++t) {
        scores(t);
        if (t * AP_BK + r < nvalid) {
#pragma unroll
            for (int st = 0; st < AP_NST; ++st)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float s = acc[st][e];
                    const float mn = fmaxf(m[st][e], s);
                    l[st][e] = l[st][e] * __builtin_amdgcn_exp2f(m[st][e] - mn) + __builtin_amdgcn_exp2f(s - mn);
                    m[st][e] = mn;
                }
        }
    }
    // the 32 lanes of a half hold the same rows: reduce over them (lane 0 always holds a valid key, so the row max is finite)
#pragma unroll
    for (int st = 0; st < AP_NST; ++st)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            float mr = m[st][e];
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) mr = fmaxf(mr, __shfl_xor(mr, d, 64));
            float lr = l[st][e] * __builtin_amdgcn_exp2f(m[st][e] - mr);  // a lane without valid keys: 0 * exp2(-inf) = 0
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) lr += __shfl_xor(lr, d, 64);
            m[st][e] = mr;
            l[st][e] = 1.0f / lr;
        }

    // ---- pass 2: recompute and store
    for (int t = 0; t < nt; ++t) {
        const int j = t * AP_BK + r;
        if (t < ntv) {
            scores(t);
#pragma unroll
            for (int st = 0; st < AP_NST; ++st)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[st][e] = j < nvalid ? __builtin_amdgcn_exp2f(acc[st][e] - m[st][e]) * l[st][e] : 0.0f;
        } else {
#pragma unroll
            for (int st = 0; st < AP_NST; ++st)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[st][e] = 0.0f;
        }
        if (j < T) {
#pragma unroll
            for (int st = 0; st < AP_NST; ++st)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int i = i0 + 32 * st + 8 * (e >> 2) + 4 * h + (e & 3);
                    if (i < T) probs[(((long)b * kHeads + head) * T + i) * T + j] = acc[st][e];
                }
        }
    }
}

hipError_t launch_attention_probs(const float* qkv, const _Float16* qhi, const _Float16* qlo, const _Float16* khi, const _Float16* klo,
                                  const float* qp, const int32_t* frames, float* probs, int B, int T, int terms, hipStream_t s) {
    if (B <= 0 || T <= 0 || B > 65535) return hipErrorInvalidValue;
    const bool f16 = qhi != nullptr;
    if (f16 ? (!qlo || !khi || !klo || (terms != 2 && terms != 3)) : !qkv) return hipErrorInvalidValue;
    const int nqb = (T + AP_BQ - 1) / AP_BQ;
    const long nblk = (long)nqb * kHeads * B;
    if (nblk > 0x7fffffffL) return hipErrorInvalidValue;
    if (f16)
        hipLaunchKernelGGL(attention_probs_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, s, nullptr, qhi, qlo, khi, klo, qp, frames,
                           probs, T, nqb, terms);
    else
        hipLaunchKernelGGL(attention_probs_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, s, qkv, nullptr, nullptr, nullptr, nullptr, qp,
                           frames, probs, T, nqb, 3);
    return hipGetLastError();
}

}  // namespace loco
