// Kernels of the SpeechT5 text decoder (HF modeling_speecht5.py: SpeechT5TextDecoderPrenet, SpeechT5DecoderLayer,
// SpeechT5TextDecoderPostnet) -- everything the decode step needs that the encoder's library did not have:
//   skinny_gemm_kernel     C[M,N] = epi(A W^T + bias) for M <= 64 rows: weight streaming, exact fp32 FMAs
//   dec_attention_kernel   fp32 attention without a bias table, per-clip key count, causal offset, key range split over waves
//   dec_attention_combine  fixed-order merge of the (max, sum, partial O) triples of the splits
//   dec_embed_kernel       token embedding + sinusoid position (teacher-forced rows and the step's single row)
//   dec_select_kernel      argmax of the step's logits + finished / pad bookkeeping + append to the token buffer
// One decode step is weight- and KV-bandwidth-bound (226 MB of fp32 weights for 2 * 226 M * B FLOP): nothing here uses the matrix
// cores.  No kernel allocates, synchronises or depends on the host; all are capturable.
// What these kernels share with the slot pool, the scores and the probabilities (argmax, score product, softmax tile, position
// rule) is decoder_common.h's; the wave reductions are loco_kernels.h's.
#include "decoder_common.h"

namespace loco {

namespace {

constexpr int kSkinnyThreads = 256;
constexpr int kSkinnyMT = 4;   // activation rows held in registers per pass
constexpr int kSkinnyNC = 2;   // weight rows (output columns) per wave
constexpr int kSkinnyKC = 256; // k elements per wave-wide 16-byte load

// A wave owns kSkinnyNC weight rows and every ks-th 256-element chunk of K: lane l holds elements 4l .. 4l+3 of a chunk (one
// coalesced 1 KiB load per weight row and chunk), multiplies them into kSkinnyMT activation rows (A is at most 64 x 3072 floats: it
// stays in L2 / L1, the weights are what comes from HBM, each element once), and keeps one partial sum per lane -- K / 64 / ks
// products each -- so that the longest rounding chain is a few dozen terms before the butterfly (K = 3072 meets the 5e-6 bar
// of the operator tests with that blocking).  The ks waves of a column group meet in LDS and are added in slice order.
// Workgroup = 4 waves = (4 / ks) column groups; grid.x covers N, grid.y blocks of 64 rows.
// ROWS (the slot pool's q | k|v product): row m of the C2 part goes to cache row c2_rows[m] of its own clip (C2 + m ldc2 + c2_rows[m]
// c2_row_stride) and is dropped when c2_rows[m] < 0 -- the destination row comes from the device, not from a host scalar.
template <int EPI, bool ROWS = false>
__global__ __launch_bounds__(kSkinnyThreads) void skinny_gemm_kernel(const float* __restrict__ A, long lda, const float* __restrict__ W,
                                                                     long ldw, const float* __restrict__ bias,
                                                                     const float* __restrict__ R, long ldr, float* __restrict__ C,
                                                                     long ldc, float* __restrict__ C2, long ldc2, int nsplit, int M,
                                                                     int N, int K, int ks, const int32_t* __restrict__ c2_rows = nullptr,
                                                                     long c2_row_stride = 0) {
    __shared__ float red[4][kSkinnyMT * kSkinnyNC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = wave % ks, group = wave / ks, groups = 4 / ks;
    const int n0 = (blockIdx.x * groups + group) * kSkinnyNC;
    const int m_begin = blockIdx.y * 64, m_end = min(M, m_begin + 64);
    const int chunks = K / kSkinnyKC;
    const float* w[kSkinnyNC];
#pragma unroll
    for (int c = 0; c < kSkinnyNC; ++c) w[c] = W + (long)min(n0 + c, N - 1) * ldw + 4 * lane;  // clamped: never read past row N - 1
    for (int m0 = m_begin; m0 < m_end; m0 += kSkinnyMT) {
        const float* a[kSkinnyMT];
#pragma unroll
        for (int r = 0; r < kSkinnyMT; ++r) a[r] = A + (long)min(m0 + r, M - 1) * lda + 4 * lane;
        float acc[kSkinnyMT][kSkinnyNC];
#pragma unroll
        for (int r = 0; r < kSkinnyMT; ++r)
#pragma unroll
            for (int c = 0; c < kSkinnyNC; ++c) acc[r][c] = 0.f;
        int c2_row = 0;  // ROWS: read before the K loop, so that the epilogue does not wait for it
        if (ROWS) c2_row = c2_rows[min(m0 + (lane % (kSkinnyMT * kSkinnyNC)) / kSkinnyNC, M - 1)];
        for (int ch = slice; ch < chunks; ch += ks) {
            const int k = ch * kSkinnyKC;
            f32x4 wv[kSkinnyNC], av[kSkinnyMT];
#pragma unroll
            for (int c = 0; c < kSkinnyNC; ++c) wv[c] = *reinterpret_cast<const f32x4*>(w[c] + k);
#pragma unroll
            for (int r = 0; r < kSkinnyMT; ++r) av[r] = *reinterpret_cast<const f32x4*>(a[r] + k);
#pragma unroll
            for (int r = 0; r < kSkinnyMT; ++r)
#pragma unroll
                for (int c = 0; c < kSkinnyNC; ++c) {
                    float t = acc[r][c];
                    t = fmaf(av[r].x, wv[c].x, t);
                    t = fmaf(av[r].y, wv[c].y, t);
                    t = fmaf(av[r].z, wv[c].z, t);
                    t = fmaf(av[r].w, wv[c].w, t);
                    acc[r][c] = t;
                }
        }
#pragma unroll
        for (int r = 0; r < kSkinnyMT; ++r)
#pragma unroll
            for (int c = 0; c < kSkinnyNC; ++c) {
                const float t = wave_sum(acc[r][c]);
                if (lane == 0) red[wave][r * kSkinnyNC + c] = t;
            }
        __syncthreads();
        if (slice == 0 && lane < kSkinnyMT * kSkinnyNC) {
            const int r = lane / kSkinnyNC, c = lane % kSkinnyNC;
            const int m = m0 + r, n = n0 + c;
            if (m < m_end && n < N) {
                float v = red[wave][lane];
                for (int q = 1; q < ks; ++q) v += red[wave + q][lane];  // slice order
                if (bias) v += bias[n];
                if (EPI == kEpiGelu) v = gelu_erf(v);
                if (EPI == kEpiResidual) v += R[(long)m * ldr + n];
                if (n < nsplit)
                    C[(long)m * ldc + n] = v;
                else if (!ROWS)
                    C2[(long)m * ldc2 + (n - nsplit)] = v;
                else if (c2_row >= 0)
                    C2[(long)m * ldc2 + (long)c2_row * c2_row_stride + (n - nsplit)] = v;
            }
        }
        __syncthreads();
    }
}

// ---- attention -------------------------------------------------------------------------------------------------------------
// One wave per (clip, head, query, key split).  Per tile of 64 keys: lane j forms q . k_j (q lives in registers, every lane reads
// its own 256-byte key row), the wave takes the tile's maximum and sum, then lane d accumulates O[d] += p_j V[j][d] with V rows
// read coalesced and p_j broadcast from lane j.  Online softmax across tiles.  Key j is visible to query i iff j < kcount[b] and
// j <= i + causal_offset.  With nsplit > 1 the wave writes (max, sum, unnormalised O) and dec_attention_combine merges the
// splits in split order.
struct DecAttnArgs {
    const float* q;
    const float* k;
    const float* v;
    const int32_t* kcount;  // [B] or null = Tk
    float* out;
    float* part;  // [units][nsplit][66] when nsplit > 1
    long ldq, ldk, ldv, ldo;      // row strides (floats); head h at column 64 h
    long sq, sk, sv, so;          // clip strides (floats)
    int B, Sq, Tk, causal_offset, causal, nsplit, keys_per_split;
    float scale;
};

__global__ __launch_bounds__(256) void dec_attention_kernel(DecAttnArgs a) {
    const int lane = threadIdx.x & 63;
    const long unit = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long units = (long)a.B * kHeads * a.Sq * a.nsplit;
    if (unit >= units) return;  // whole waves leave: no barrier below
    const int sp = (int)(unit % a.nsplit);
    const long row = unit / a.nsplit;
    const auto [i, h, b] = dec_attn_row(row, a.Sq);
    const int nvis = dec_visible_keys(a.kcount, b, a.Tk, a.causal, i, a.causal_offset);
    const int j_begin = sp * a.keys_per_split, j_end = min(nvis, j_begin + a.keys_per_split);

    const float* qp = a.q + (long)b * a.sq + (long)i * a.ldq + h * kHeadDim;
    LOCO_DEC_LOAD_Q(q, qp, a.scale);
    const float* kb = a.k + (long)b * a.sk + h * kHeadDim;
    const float* vb = a.v + (long)b * a.sv + h * kHeadDim;

    float m_run = -INFINITY, s_run = 0.f, o = 0.f;
    for (int j0 = j_begin; j0 < j_end; j0 += 64) {
        const int j = j0 + lane;
        float sc = -INFINITY;
        if (j < j_end) {
            const float* kr = kb + (long)j * a.ldk;
            LOCO_DEC_QK(sc, q, kr);
        }
        LOCO_DEC_SOFTMAX_TILE(sc, j < j_end, m_run, s_run, m_new, p, corr);
        o *= corr;
        const int nj = min(64, j_end - j0);
        for (int jj = 0; jj < nj; ++jj) {
            const float pj = __shfl(p, jj, 64);
            o = fmaf(pj, vb[(long)(j0 + jj) * a.ldv + lane], o);
        }
        m_run = m_new;
    }
    if (a.nsplit == 1) {
        a.out[(long)b * a.so + (long)i * a.ldo + h * kHeadDim + lane] = s_run > 0.f ? o / s_run : 0.f;
    } else {
        float* pr = a.part + unit * 66;
        pr[2 + lane] = o;
        if (lane == 0) {
            pr[0] = m_run;
            pr[1] = s_run;
        }
    }
}

__global__ __launch_bounds__(256) void dec_attention_combine(DecAttnArgs a) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)a.B * kHeads * a.Sq) return;
    const auto [i, h, b] = dec_attn_row(row, a.Sq);
    const float* pr = a.part + row * a.nsplit * 66;
    float m = -INFINITY;
    for (int s = 0; s < a.nsplit; ++s) m = fmaxf(m, pr[s * 66]);
    float sum = 0.f, o = 0.f;
    for (int s = 0; s < a.nsplit; ++s) {  // split order
        const float ms = pr[s * 66];
        if (ms == -INFINITY) continue;  // a split without a visible key
        const float w = expf(ms - m);
        sum = fmaf(pr[s * 66 + 1], w, sum);
        o = fmaf(pr[s * 66 + 2 + lane], w, o);
    }
    a.out[(long)b * a.so + (long)i * a.ldo + h * kHeadDim + lane] = sum > 0.f ? o / sum : 0.f;
}

// ---- prenet ----------------------------------------------------------------------------------------------------------------
// x[b, s, :] = embed[ids[b, s]] + table[pos], pos = (non-pad tokens of row b up to and including s) + 1 for a token, 1 (the zero
// row) for <pad> (HF :337-351 with padding_idx 1).  Teacher-forced form: one workgroup per (b, s), the count is taken over the row.
__global__ __launch_bounds__(256) void dec_embed_kernel(const int32_t* __restrict__ ids, long ld_ids, const float* __restrict__ embed,
                                                        int vocab, const float* __restrict__ table, int table_rows, float* __restrict__ x,
                                                        int S, int32_t* __restrict__ positions) {
    __shared__ int part[4];
    const int s = blockIdx.x, b = blockIdx.y;
    const int32_t* row = ids + (long)b * ld_ids;
    int cnt = 0;
    for (int t = threadIdx.x; t <= s; t += 256) cnt += row[t] != kDecPadToken;
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    cnt = part[0] + part[1] + part[2] + part[3];
    const int pos = dec_embed_row(row[s], row[s] != kDecPadToken, cnt, embed, vocab, table, table_rows, x + ((long)b * S + s) * kHidden);
    if (positions && threadIdx.x == 0) positions[(long)b * S + s] = pos;
}

// The step's form: token t of every row from the token buffer; the running non-pad count is kept per position (nonpad[b, t] =
// tokens != <pad> among positions 0 .. t), so that a step only reads what earlier steps wrote and can be replayed.
__global__ __launch_bounds__(256) void dec_embed_step_kernel(const int32_t* __restrict__ tokens, int S_max, int t,
                                                             const float* __restrict__ embed, int vocab, const float* __restrict__ table,
                                                             int table_rows, int32_t* __restrict__ nonpad, float* __restrict__ x) {
    const int b = blockIdx.x;
    const int raw = tokens[(long)b * S_max + t];
    const bool token = raw != kDecPadToken;
    const int cnt = (t == 0 ? 0 : nonpad[(long)b * S_max + t - 1]) + token;
    if (threadIdx.x == 0) nonpad[(long)b * S_max + t] = cnt;
    dec_embed_row(raw, token, cnt, embed, vocab, table, table_rows, x + (long)b * kHidden);
}

// ---- token selection -------------------------------------------------------------------------------------------------------
// One workgroup, thread b = row b (B <= 64 = one wave).  argmax by decoder_common.h's rule in an ascending serial scan: the candidate's
// index is always above the incumbent's, so argmax_better(v, n, bv, best) reduces to v > bv || (v != v && bv == bv): the scan spells
// that out (the compiler does not reduce the call).  A finished row
// takes <pad>; a row that emits <eos> is finished from the next step on (finished[b, p] = row b is finished once position p is
// written: a step reads position t and writes t + 1, so it can be replayed); state[0] = rows still unfinished after this step.
__global__ __launch_bounds__(64) void dec_select_kernel(const float* __restrict__ logits, int vocab, int B, int32_t* __restrict__ tokens,
                                                        int S_max, int t, int32_t* __restrict__ finished, int32_t* __restrict__ lengths,
                                                        int32_t* __restrict__ state, int eos, int pad) {
    const int b = threadIdx.x;
    int open = 0;
    if (b < B) {
        const float* l = logits + (long)b * vocab;
        int best = 0;
        float bv = l[0];
        for (int n = 1; n < vocab; ++n) {
            const float v = l[n];
            if (v > bv || (v != v && bv == bv)) {  // argmax_better(v, n, bv, best) with n > best
                bv = v;
                best = n;
            }
        }
        const int fin = t == 0 ? 0 : finished[(long)b * S_max + t];
        const int tok = fin ? pad : best;
        tokens[(long)b * S_max + t + 1] = tok;
        const int fin_new = fin | (tok == eos);
        finished[(long)b * S_max + t + 1] = fin_new;
        if (!fin) lengths[b] = t + 2;  // tokens of this row including the one just written
        open = !fin_new;
    }
    const unsigned long long any = __ballot(open);
    if (threadIdx.x == 0) {
        state[0] = __popcll(any);
        state[1] = t + 1;  // steps completed
    }
}

__global__ void dec_begin_kernel(int32_t* __restrict__ tokens, int B, int S_max, int start, int pad, int32_t* __restrict__ lengths,
                                 int32_t* __restrict__ state) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)B * S_max; i += (long)gridDim.x * blockDim.x)
        tokens[i] = (i % S_max) == 0 ? start : pad;
    if (blockIdx.x == 0 && (int)threadIdx.x < B) lengths[threadIdx.x] = 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state[0] = B;
        state[1] = 0;
    }
}

}  // namespace

int skinny_gemm_slices(int N, int K) {
    // enough workgroups to keep 256 CUs loading: 2 columns per workgroup when K is long (FFN2, 12 chunks: 4 slices of 3),
    // 4 columns otherwise (768 = 3 chunks: 2 slices, lm_head's N = 81 included: 21 workgroups); a narrow N with K >= 1024 takes 4 slices
    const int chunks = K / kSkinnyKC;
    if (chunks >= 8 || (N <= 128 && chunks >= 4)) return 4;
    if (chunks >= 2) return 2;
    return 1;
}

hipError_t launch_skinny_gemm(const float* A, long lda, const float* W, long ldw, const float* bias, const float* R, long ldr, float* C,
                              long ldc, float* C2, long ldc2, int nsplit, int M, int N, int K, int epilogue, hipStream_t s) {
    if (M <= 0 || N <= 0 || K <= 0 || K % kSkinnyKC != 0) return hipErrorInvalidValue;
    if ((lda | ldw) & 3) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W)) & 15) return hipErrorInvalidValue;
    if (!C || (epilogue == kEpiResidual && !R)) return hipErrorInvalidValue;
    if (!C2) nsplit = N;
    const int ks = skinny_gemm_slices(N, K), cols = (4 / ks) * kSkinnyNC;
    const dim3 grid((unsigned)((N + cols - 1) / cols), (unsigned)((M + 63) / 64)), block(kSkinnyThreads);
    switch (epilogue) {
        case kEpiNone:
            hipLaunchKernelGGL((skinny_gemm_kernel<kEpiNone>), grid, block, 0, s, A, lda, W, ldw, bias, R, ldr, C, ldc, C2, ldc2, nsplit, M, N, K, ks);
            break;
        case kEpiGelu:
            hipLaunchKernelGGL((skinny_gemm_kernel<kEpiGelu>), grid, block, 0, s, A, lda, W, ldw, bias, R, ldr, C, ldc, C2, ldc2, nsplit, M, N, K, ks);
            break;
        case kEpiResidual:
            hipLaunchKernelGGL((skinny_gemm_kernel<kEpiResidual>), grid, block, 0, s, A, lda, W, ldw, bias, R, ldr, C, ldc, C2, ldc2, nsplit, M, N, K, ks);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_skinny_gemm_rows(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, float* C2,
                                   long ldc2, const int32_t* c2_rows, long c2_row_stride, int nsplit, int M, int N, int K, hipStream_t s) {
    if (M <= 0 || M > kSkinnyMaxM || N <= 0 || K <= 0 || K % kSkinnyKC != 0 || nsplit < 0 || nsplit > N) return hipErrorInvalidValue;
    if ((lda | ldw) & 3) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W)) & 15) return hipErrorInvalidValue;
    if (!C || !C2 || !c2_rows) return hipErrorInvalidValue;
    const int ks = skinny_gemm_slices(N, K), cols = (4 / ks) * kSkinnyNC;
    const dim3 grid((unsigned)((N + cols - 1) / cols), 1), block(kSkinnyThreads);
    hipLaunchKernelGGL((skinny_gemm_kernel<kEpiNone, true>), grid, block, 0, s, A, lda, W, ldw, bias, nullptr, 0, C, ldc, C2, ldc2, nsplit, M, N, K, ks,
                       c2_rows, c2_row_stride);
    return hipGetLastError();
}

// Key splits of one attention launch: a pure function of the shape (so that a step is reproducible), at most ceil(Tk / 256)
// and at most kDecAttnMaxSplit of them (a split's key range is a multiple of 64 and never shorter than 128 keys), enough waves for ~4 per SIMD of the chip when the key range allows it.
int dec_attention_splits(int B, int Sq, int Tk) {
    const long rows = (long)B * kHeads * Sq;
    long want = (4096 + rows - 1) / rows;
    const long by_keys = (Tk + 255) / 256;  // no split shorter than 256 keys
    if (want > by_keys) want = by_keys;
    if (want > kDecAttnMaxSplit) want = kDecAttnMaxSplit;
    return want < 1 ? 1 : (int)want;
}

size_t dec_attention_scratch_bytes(int B, int Sq, int Tk) {
    const int ns = dec_attention_splits(B, Sq, Tk);
    return ns > 1 ? (size_t)B * kHeads * Sq * ns * 66 * sizeof(float) : 0;
}

hipError_t launch_dec_attention(const float* q, long ldq, long sq, const float* k, long ldk, long sk, const float* v, long ldv, long sv,
                                const int32_t* kcount, float* out, long ldo, long so, int B, int Sq, int Tk, int causal, int causal_offset,
                                float scale, float* scratch, hipStream_t s) {
    if (B <= 0 || Sq <= 0 || Tk <= 0 || !q || !k || !v || !out) return hipErrorInvalidValue;
    if ((ldq | ldk | sq | sk) & 3) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return hipErrorInvalidValue;
    DecAttnArgs a{};
    a.q = q, a.k = k, a.v = v, a.kcount = kcount, a.out = out, a.part = scratch;
    a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.ldo = ldo, a.sq = sq, a.sk = sk, a.sv = sv, a.so = so;
    a.B = B, a.Sq = Sq, a.Tk = Tk, a.causal = causal, a.causal_offset = causal_offset, a.scale = scale;
    a.nsplit = dec_attention_splits(B, Sq, Tk);
    if (a.nsplit > 1 && !scratch) return hipErrorInvalidValue;
    a.keys_per_split = ((Tk + a.nsplit - 1) / a.nsplit + 63) / 64 * 64;
    const long rows = (long)B * kHeads * Sq, units = rows * a.nsplit;
    if (units > 0x7fffffffL * 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_attention_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, a);
    if (a.nsplit > 1) hipLaunchKernelGGL(dec_attention_combine, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// The slot pool's attention (one query per slot): split s covers keys [256 s, 256 s + 256) whatever the launch's key bound is, and the
// splits are merged in split order with empty ones skipped, so a slot's output is a pure function of its own key count -- not of the
// slots beside it nor of the bound the host sized the launch by.  One launched split writes its result directly: the same bits as the
// merge of one split (weight exp(0) = 1).  Tk_bound >= every kcount[b] that is to be seen in full; scratch >= dec_pool_attention_scratch_bytes.
int dec_pool_attention_splits(int Tk_bound) { return Tk_bound <= kDecPoolSplitKeys ? 1 : (Tk_bound + kDecPoolSplitKeys - 1) / kDecPoolSplitKeys; }

size_t dec_pool_attention_scratch_bytes(int slots, int Tk_bound) {
    return (size_t)slots * kHeads * dec_pool_attention_splits(Tk_bound) * 66 * sizeof(float);
}

hipError_t launch_dec_pool_attention(const float* q, const float* k, long ldk, long sk, const float* v, const int32_t* kcount, float* out,
                                     int slots, int Tk_bound, float* scratch, hipStream_t s) {
    if (slots <= 0 || slots > kSkinnyMaxM || Tk_bound <= 0 || !q || !k || !v || !out || !kcount || !scratch) return hipErrorInvalidValue;
    if ((ldk | sk) & 3) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return hipErrorInvalidValue;
    DecAttnArgs a{};
    a.q = q, a.k = k, a.v = v, a.kcount = kcount, a.out = out, a.part = scratch;
    a.ldq = kHidden, a.ldk = ldk, a.ldv = ldk, a.ldo = kHidden, a.sq = kHidden, a.sk = sk, a.sv = sk, a.so = kHidden;
    a.B = slots, a.Sq = 1, a.Tk = Tk_bound, a.causal = 0, a.causal_offset = 0, a.scale = 1.0f;
    a.nsplit = dec_pool_attention_splits(Tk_bound);
    a.keys_per_split = kDecPoolSplitKeys;
    const long rows = (long)slots * kHeads, units = rows * a.nsplit;
    hipLaunchKernelGGL(dec_attention_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, a);
    if (a.nsplit > 1) hipLaunchKernelGGL(dec_attention_combine, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_dec_embed(const int32_t* ids, long ld_ids, const float* embed, int vocab, const float* table, int table_rows, float* x,
                            int B, int S, int32_t* positions, hipStream_t s) {
    if (B <= 0 || S <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_embed_kernel, dim3(S, B), dim3(256), 0, s, ids, ld_ids, embed, vocab, table, table_rows, x, S, positions);
    return hipGetLastError();
}

hipError_t launch_dec_embed_step(const int32_t* tokens, int S_max, int t, const float* embed, int vocab, const float* table, int table_rows,
                                 int32_t* nonpad, float* x, int B, hipStream_t s) {
    hipLaunchKernelGGL(dec_embed_step_kernel, dim3(B), dim3(256), 0, s, tokens, S_max, t, embed, vocab, table, table_rows, nonpad, x);
    return hipGetLastError();
}

hipError_t launch_dec_select(const float* logits, int vocab, int B, int32_t* tokens, int S_max, int t, int32_t* finished, int32_t* lengths,
                             int32_t* state, int eos, int pad, hipStream_t s) {
    if (B <= 0 || B > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_select_kernel, dim3(1), dim3(64), 0, s, logits, vocab, B, tokens, S_max, t, finished, lengths, state, eos, pad);
    return hipGetLastError();
}

hipError_t launch_dec_begin(int32_t* tokens, int B, int S_max, int start, int pad, int32_t* lengths, int32_t* state, hipStream_t s) {
    if (B <= 0 || B > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_begin_kernel, dim3((unsigned)(((long)B * S_max + 255) / 256)), dim3(256), 0, s, tokens, B, S_max, start, pad, lengths, state);
    return hipGetLastError();
}

}  // namespace loco
