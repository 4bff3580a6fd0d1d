// Attention probabilities of the teacher-forced decoder pass and what token timestamps are made of (include/loco_asr.h:
// loco_decoder_forward_attn, loco_decoder_align, loco_op_decoder_attention_probs, loco_op_dtw_align):
//   dec_attention_probs_kernel  P[b,h,i,:] = softmax over the visible keys of scale q.k, exact fp32, masked entries exactly 0
//   dec_attn_mean_kernel        A[b,s,t] (+)= sum over the selected heads of one layer's P; the last layer multiplies by 1 / pairs
//   dtw_align_kernel            monotone DTW over -A in double, one workgroup per clip, anti-diagonals; back-pointers in global memory
// dec_attention_kernel (decoder.hip) never forms P: it is an online-softmax kernel; what the two must agree on (row decode, visible
// keys, scaled q, the product q . k_j, the tile's max / sum / rescale) is decoder_common.h's.  The schedule here is the plain one: one wave per P
// row, two passes over the keys, every store instruction one contiguous 256-byte piece of the row.  Each P entry costs its 256-byte key
// row twice (from L2: the key rows of a head are shared by its S queries), so the kernel is bound by those reads, not by its stores:
// measured at ~90-100 x the store-byte floor of P (profiles/decoder_attn_cost.json).
// No kernel allocates, synchronises with the host or uses atomics.
#include "decoder_common.h"

namespace loco {

namespace {

struct DecProbsArgs {
    const float* q;
    const float* k;
    const int32_t* kcount;  // [B] or null = Tk
    float* P;               // [B, 12, Sq, Tk]
    long ldq, ldk, sq, sk;  // row and clip strides (floats); head h at column 64 h
    int B, Sq, Tk, causal;
    float scale;
};

// q . k_j as a function: this kernel forms it in two places
__device__ __forceinline__ float probs_score(const f32x4 (&q)[kHeadDim / 4], const float* kr) {
    float sc;
    LOCO_DEC_QK(sc, q, kr);
    return sc;
}

// One wave per (clip, head, query).  Pass 1: running maximum and sum over the visible keys in tiles of 64 (lane j of a tile owns key
// j0 + j).  Pass 2: the same products in the same order, p = exp(s - m) / l stored by the lane that owns the key; keys that are not
// visible (j >= kcount[b], or j > i when causal) are written as 0.0f and their rows are never read.
__global__ __launch_bounds__(256) void dec_attention_probs_kernel(DecProbsArgs a) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)a.B * kHeads * a.Sq) return;  // whole waves leave: no barrier below
    const auto [i, h, b] = dec_attn_row(row, a.Sq);
    const int nvis = dec_visible_keys(a.kcount, b, a.Tk, a.causal, i, 0);

    const float* qp = a.q + (long)b * a.sq + (long)i * a.ldq + h * kHeadDim;
    LOCO_DEC_LOAD_Q(q, qp, a.scale);
    const float* kb = a.k + (long)b * a.sk + h * kHeadDim;

    float m_run = -INFINITY, s_run = 0.f;
    for (int j0 = 0; j0 < nvis; j0 += 64) {
        const int j = j0 + lane;
        const float sc = j < nvis ? probs_score(q, kb + (long)j * a.ldk) : -INFINITY;
        LOCO_DEC_SOFTMAX_TILE(sc, j < nvis, m_run, s_run, m_new, p, corr);
        m_run = m_new;
    }
    float* pr = a.P + row * (long)a.Tk;  // 64-bit: B * 12 * Sq * Tk passes 2^31
    for (int j0 = 0; j0 < a.Tk; j0 += 64) {
        const int j = j0 + lane;
        float p = 0.f;
        if (j < nvis) p = expf(probs_score(q, kb + (long)j * a.ldk) - m_run) / s_run;
        if (j < a.Tk) pr[j] = p;  // the wave writes 256 contiguous bytes (the row's last tile: what is left of it)
    }
}

// A[b, s, t] = (first ? 0 : A[b, s, t]) + sum over the heads in `heads` (bit h), ascending, of P[b, h, s, t]; times inv_n when last.
__global__ __launch_bounds__(256) void dec_attn_mean_kernel(const float* __restrict__ P, float* __restrict__ A, long per_head, long total,
                                                            unsigned heads, int first, int last, float inv_n) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long b = idx / per_head, rem = idx - b * per_head;
        const float* p = P + b * kHeads * per_head + rem;
        float acc = first ? 0.f : A[idx];
#pragma unroll
        for (int h = 0; h < kHeads; ++h)
            if (heads >> h & 1u) acc += p[(long)h * per_head];
        A[idx] = last ? acc * inv_n : acc;
    }
}

constexpr int kDtwThreads = 512;  // one thread per token row: kDecAlignMaxTokens = 450 rows fit

// Monotone DTW of one clip: cost c[s,t] = -(double)A[s,t] over s < n, t < F; D[0,0] = c[0,0], D[s,t] = c[s,t] + min(D[s-1,t-1],
// D[s-1,t], D[s,t-1]) with missing neighbours +inf; ties: the diagonal first, then (s-1,t), then (s,t-1).  Thread s owns row s and
// walks it along the anti-diagonals d = s + t: its left neighbour is its own previous value (a register), the other two are row
// s - 1's values of the last two diagonals, kept in a ring of three LDS rows (one barrier per diagonal).  Every cell is one double
// add and one three-way minimum, so the result does not depend on the traversal order.  One back-pointer byte per cell goes to bp
// [S, T]; thread 0 then walks back from (n-1, F-1) and writes each token's first frame and last frame + 1.
__global__ __launch_bounds__(kDtwThreads) void dtw_align_kernel(const float* __restrict__ A, long ld, const int32_t* __restrict__ ncount,
                                                                const int32_t* __restrict__ frames, int S, int T, int32_t* __restrict__ start,
                                                                int32_t* __restrict__ end, unsigned char* __restrict__ bp_all) {
    __shared__ double ring[3][kDtwThreads];
    const int b = blockIdx.x, s = threadIdx.x;
    const int n = max(0, min(ncount[b], S));
    const int F = max(0, min(frames ? frames[b] : T, T));
    const bool run = n > 0 && F > 0;
    if (s < S && (!run || s >= n)) {
        start[(long)b * S + s] = -1;
        end[(long)b * S + s] = -1;
    }
    if (!run) return;  // the whole workgroup leaves: n and F are the same for every thread
    const double inf = INFINITY;
    ring[0][s] = ring[1][s] = ring[2][s] = inf;
    __syncthreads();
    const float* arow = A + ((long)b * S + min(s, S - 1)) * ld;
    unsigned char* bp = bp_all + ((long)b * S + min(s, S - 1)) * (long)T;
    double left = inf;
    const int last = n + F - 2;
    for (int d = 0; d <= last; ++d) {
        const int t = d - s;
        double val = inf;
        if (s < n && t >= 0 && t < F) {
            const double c = -(double)arow[t];
            if (d == 0) {
                val = c;  // (0, 0)
                bp[0] = 0;
            } else {
                const double diag = s > 0 ? ring[(d + 1) % 3][s - 1] : inf;  // diagonal d - 2
                const double up = s > 0 ? ring[(d + 2) % 3][s - 1] : inf;    // diagonal d - 1
                double best = diag;
                unsigned char from = 0;
                if (up < best) best = up, from = 1;
                if (left < best) best = left, from = 2;
                val = c + best;
                bp[t] = from;
            }
            left = val;
        }
        ring[d % 3][s] = val;
        __syncthreads();
    }
    if (s == 0) {  // the back-pointers of the other threads are visible: the last barrier orders them
        const unsigned char* bpb = bp_all + (long)b * S * (long)T;
        int32_t* st = start + (long)b * S;
        int32_t* en = end + (long)b * S;
        int i = n - 1, t = F - 1;
        en[i] = t + 1;
        while (i > 0 || t > 0) {
            unsigned char from = bpb[(long)i * T + t];
            if (i == 0) from = 2;  // what the recurrence wrote there; restated so that no input (a NaN in A) can walk out of the matrix
            else if (t == 0) from = 1;
            if (from == 2) {
                --t;
            } else {
                st[i] = t;
                --i;
                if (from == 0) --t;
                en[i] = t + 1;
            }
        }
        st[0] = 0;
    }
}

}  // namespace

hipError_t launch_dec_attention_probs(const float* q, long ldq, long sq, const float* k, long ldk, long sk, const int32_t* kcount, float* P,
                                      int B, int Sq, int Tk, int causal, float scale, hipStream_t s) {
    if (B <= 0 || Sq <= 0 || Tk <= 0 || !q || !k || !P) return hipErrorInvalidValue;
    if ((ldq | ldk | sq | sk) & 3) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return hipErrorInvalidValue;
    DecProbsArgs a{};
    a.q = q, a.k = k, a.kcount = kcount, a.P = P, a.ldq = ldq, a.ldk = ldk, a.sq = sq, a.sk = sk;
    a.B = B, a.Sq = Sq, a.Tk = Tk, a.causal = causal, a.scale = scale;
    const long rows = (long)B * kHeads * Sq;
    if (rows > 0x7fffffffL * 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_attention_probs_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_dec_attn_mean(const float* P, float* A, int B, int S, int T, unsigned heads, int first, int last, float inv_n, hipStream_t s) {
    if (B <= 0 || S <= 0 || T <= 0 || !P || !A) return hipErrorInvalidValue;
    const long per_head = (long)S * T, total = (long)B * per_head;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(dec_attn_mean_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, P, A, per_head, total, heads, first,
                       last, inv_n);
    return hipGetLastError();
}

hipError_t launch_dtw_align(const float* A, long ld, const int32_t* n, const int32_t* frames, int B, int S, int T, int32_t* start, int32_t* end,
                            unsigned char* back, hipStream_t s) {
    if (B <= 0 || S <= 0 || S > kDecAlignMaxTokens || T <= 0 || ld < T || !A || !n || !start || !end || !back) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dtw_align_kernel, dim3((unsigned)B), dim3(kDtwThreads), 0, s, A, ld, n, frames, S, T, start, end, back);
    return hipGetLastError();
}

}  // namespace loco
