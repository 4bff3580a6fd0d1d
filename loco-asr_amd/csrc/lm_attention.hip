// GPT-2 language model with a cached context: attention over "cached prefix + own causal tokens", and the small kernels of the K/V cache.
//
//   lm_ctx_attention   out[n, t, head, :] = softmax_j(q . k_j / 8) v_j over the slot's cached keys j < P[n] (all visible) and the sequence's
//                      own keys t' <= t.  P[n] = 0 is plain causal attention, so the same kernel prefills a slot.
//   lm_ctx_embed       x[row0[n] + t, :] = wte[tokens[tok0[n] + t]] + wpe[P[n] + t]
//   lm_ctx_append      the committing sequences' k | v rows of one layer -> their slots, at positions P[n] + t
//   lm_ctx_gather      the rows that are scored: token t of a sequence is predicted from row t - 1, token 0 from the slot's stored last row
//   lm_ctx_last        the committing sequences' last residual row -> their slots
//
// ---- lm_ctx_attention ----------------------------------------------------------------------------------------------------------------
// launch_dec_attention spends one wave per (row, head, query) and streams every key row from memory for that query alone.  Here a
// workgroup owns a tile of 128 queries of ONE sequence and one head (4 waves x 32 queries) and walks the keys in tiles of 64: every K and V
// tile is staged in LDS once (K rows padded to 68 floats, attention_f32.hip's layout) and read from there by all four waves, so key / value
// traffic per layer falls by the number of query rows a tile holds.  Products are v_mfma_f32_32x32x2_f32 in attention_f32.hip's
// orientation: S^T = K Q^T puts the query on the lane and 2 x 16 keys of the tile in its registers, the online softmax (fp32, log2 domain)
// is lane-local plus one exchange with lane ^ 32, and P^T is the B operand of O^T = V^T P^T as it stands.
//
// The promise: a sequence's output is a function of its own rows, its slot's contents and P[n] alone, bit for bit -- not of N, of the
// sequences beside it, of the slot's index or of its place in the launch.
//   * prefix tiles start at key 0 of the slot, own tiles at the sequence's first row, and a query tile never spans two sequences: query
//     t is always lane t % 32 of wave (t / 32) % 4, and key j of either part always sits in the same tile at the same place;
//   * tiles are walked in one order (prefix ascending, then own ascending), and the running (max, sum, O) has one written update;
//   * a tile whose keys are all masked for a wave's queries changes nothing (alpha = 1, p = 0), so skipping it -- own tiles past the
//     wave's last query -- leaves the bits alone.
// Keys past an end are never read: their addresses are clamped to the last valid row of the part, and their scores enter as -inf.  A
// query always sees its own key, so no valid row is empty.  Rows t >= len[n] of a partly filled tile are computed on clamped addresses and
// not stored.  Short sequences leave MFMA rows (and whole waves) unused; that is the price of the promise.
//
// LDS: 64 x 68 + 64 x 64 floats = 33 792 bytes, single-buffered (the next tile's global loads are in flight in registers while this one is
// consumed); four workgroups fit a CU's 160 KiB, __launch_bounds__(256, 2) asks for two (8 waves per CU, up to 256 VGPRs each).
#include <math.h>

#include "loco_kernels.h"

namespace loco {

namespace {

constexpr int LC_BQ = 128;
constexpr int LC_BK = 64;
constexpr int LC_LDK = kHeadDim + 4;

__global__ __launch_bounds__(256, 2) void lm_ctx_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ kcache,
                                                                  const float* __restrict__ vcache, long slot_stride, const LmCtxSeqs seqs,
                                                                  float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float kl[LC_BK * LC_LDK];
    __shared__ __attribute__((aligned(16))) float vl[LC_BK * kHeadDim];

    const int n = blockIdx.y;
    const int qt = blockIdx.x / kHeads, head = blockIdx.x - qt * kHeads;
    const int len = seqs.len[n];
    const int q0 = qt * LC_BQ;
    if (q0 >= len) return;  // the grid is sized by the longest sequence
    const int P = seqs.P[n];
    const long row0 = seqs.row0[n];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int iw0 = q0 + wave * 32;  // first query of this wave
    const int t = iw0 + r;
    const int tc = t < len ? t : len - 1;
    const bool wave_active = iw0 < len;

    const float* own = qkv + row0 * kQkv + head * kHeadDim;
    const float* kpre = kcache + (long)seqs.slot[n] * slot_stride + head * kHeadDim;
    const float* vpre = vcache + (long)seqs.slot[n] * slot_stride + head * kHeadDim;

    // Q fragment (B operand of S^T = K Q^T): q[tc][32 h + kk] / 8, in the log2 domain
    constexpr float kQScale = 0.125f * 1.4426950408889634f;
    float q[32];
    {
        const f32x4* qr = reinterpret_cast<const f32x4*>(own + (long)tc * kQkv + 32 * h);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 v = qr[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) q[4 * i + e] = v[e] * kQScale;
        }
    }

    const int ntp = (P + LC_BK - 1) / LC_BK;
    const int own_end = min(len, q0 + LC_BQ);  // own keys this query tile can see
    const int nt = ntp + (own_end + LC_BK - 1) / LC_BK;

    // staging map: 16-byte piece f = tid + 256 u -> key row f / 16, 4-float column f % 16
    const int srow = tid >> 4, sc4 = (tid & 15) * 4;
    f32x4 pk[4], pv[4];
    auto gload = [&](int tile) {
        const bool pre = tile < ntp;
        const int j0 = (pre ? tile : tile - ntp) * LC_BK;
        const int last = (pre ? P : len) - 1;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int j = j0 + srow + 16 * u;
            j = j < last ? j : last;
            const float* kp = pre ? kpre + (long)j * kHidden : own + (long)j * kQkv + kHidden;
            const float* vp = pre ? vpre + (long)j * kHidden : own + (long)j * kQkv + 2 * kHidden;
            pk[u] = *reinterpret_cast<const f32x4*>(kp + sc4);
            pv[u] = *reinterpret_cast<const f32x4*>(vp + sc4);
        }
    };

    f32x16 o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    gload(0);
    for (int tile = 0; tile < nt; ++tile) {
        __syncthreads();  // every wave is done with the previous tile
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            *reinterpret_cast<f32x4*>(kl + (srow + 16 * u) * LC_LDK + sc4) = pk[u];
            *reinterpret_cast<f32x4*>(vl + (srow + 16 * u) * kHeadDim + sc4) = pv[u];
        }
        __syncthreads();
        if (tile + 1 < nt) gload(tile + 1);

        const bool pre = tile < ntp;
        const int j0 = (pre ? tile : tile - ntp) * LC_BK;
        if (!wave_active || (!pre && j0 > iw0 + 31)) continue;  // wave-uniform: nothing of this tile is visible to these 32 queries

        // ---- S^T = K Q^T: s[st][e] = score of key j0 + 32 st + 8 (e >> 2) + 4 h + (e & 3) for query t
        // Blocked accumulation (gemm_f32.hip does the same): the instruction rounds after each of its two products, so one chain over
        // the 64 head dimensions is 64 roundings at the size of the partial sums -- measured 1.5e-6 on scores of order one, 1.3 x the
        // per-row bar of the parity test.  Four chains of 16 dimensions each, added pairwise, stay at a third of it.
        f32x16 s[2];
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            f32x16 part[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
                for (int e = 0; e < 16; ++e) part[b][e] = 0.f;
#pragma unroll
                for (int c = 2 * b; c < 2 * b + 2; ++c) {
                    const f32x4 kf = *reinterpret_cast<const f32x4*>(kl + (32 * st + r) * LC_LDK + 32 * h + 4 * c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) part[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], q[4 * c + e], part[b], 0, 0, 0);
                }
            }
            s[st] = (part[0] + part[1]) + (part[2] + part[3]);
        }
        // ---- mask: prefix keys j < P, own keys j <= t
        const int lim = pre ? P - 1 : t;
        float mx = -INFINITY;
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int j = j0 + 32 * st + 8 * (e >> 2) + 4 * h + (e & 3);
                const float x = j <= lim ? s[st][e] : -INFINITY;
                s[st][e] = x;
                mx = fmaxf(mx, x);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));

        // ---- online softmax: the query's row lives on lanes r and r + 32
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
#pragma unroll
        for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
        float ps = 0.f;
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = __builtin_amdgcn_exp2f(s[st][e] - m_new);
                s[st][e] = p;
                ps += p;
            }
        l_run = l_run * alpha + ps;

        // ---- O^T += V^T P^T: o0[e] / o1[e] = O[t][8 (e >> 2) + 4 h + (e & 3)] / [32 + ...]
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float* vr = vl + (32 * st + 8 * (e >> 2) + 4 * h + (e & 3)) * kHeadDim + r;
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], s[st][e], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], s[st][e], o1, 0, 0, 0);
            }
    }

    if (t >= len) return;
    const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32, 64));
    float* orow = out + (row0 + t) * kHidden + head * kHeadDim + 4 * h;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
        *reinterpret_cast<f32x4*>(orow + 8 * g4) = f32x4{o0[4 * g4] * inv, o0[4 * g4 + 1] * inv, o0[4 * g4 + 2] * inv, o0[4 * g4 + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 32 + 8 * g4) = f32x4{o1[4 * g4] * inv, o1[4 * g4 + 1] * inv, o1[4 * g4 + 2] * inv, o1[4 * g4 + 3] * inv};
    }
}

// the sequence that owns packed row m (rows are laid out in sequence order): n, and t = m - row0[n]
__device__ __forceinline__ int lm_ctx_find(const LmCtxSeqs& seqs, int m, int& t) {
    int n = 0;
    while (n + 1 < seqs.n && m >= seqs.row0[n + 1]) ++n;
    t = m - seqs.row0[n];
    return n;
}

__global__ __launch_bounds__(192) void lm_ctx_embed_kernel(const int32_t* __restrict__ tokens, const LmCtxSeqs seqs, const float* __restrict__ wte,
                                                           int V, const float* __restrict__ wpe, float* __restrict__ x, int32_t* status) {
    int t;
    const int n = lm_ctx_find(seqs, blockIdx.x, t);
    const long pos = (long)seqs.tok0[n] + t;
    const int id = tokens[pos];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (id >= 0 && id < V) {
        v = reinterpret_cast<const f32x4*>(wte + (long)id * kHidden)[threadIdx.x] +
            reinterpret_cast<const f32x4*>(wpe + (long)(seqs.P[n] + t) * kHidden)[threadIdx.x];
    } else if (threadIdx.x == 0 && status) {
        atomicMin(status, (int)min(pos, (long)0x7ffffffe));
    }
    reinterpret_cast<f32x4*>(x + (long)blockIdx.x * kHidden)[threadIdx.x] = v;
}

// 384 threads: one 16-byte piece of the row's k | v each
__global__ __launch_bounds__(384) void lm_ctx_append_kernel(const float* __restrict__ qkv, const LmCtxSeqs seqs, float* __restrict__ kcache,
                                                            float* __restrict__ vcache, long slot_stride) {
    int t;
    const int n = lm_ctx_find(seqs, blockIdx.x, t);
    if (!(seqs.flags[n] & kLmCtxCommit)) return;
    const int piece = threadIdx.x < 192 ? threadIdx.x : threadIdx.x - 192;
    const bool is_v = threadIdx.x >= 192;
    const f32x4 v = reinterpret_cast<const f32x4*>(qkv + (long)blockIdx.x * kQkv + (is_v ? 2 : 1) * kHidden)[piece];
    float* dst = (is_v ? vcache : kcache) + (long)seqs.slot[n] * slot_stride + (long)(seqs.P[n] + t) * kHidden;
    reinterpret_cast<f32x4*>(dst)[piece] = v;
}

// scored row r (the scoring sequences' tokens, flat in sequence order): its hidden row and its target
__global__ __launch_bounds__(192) void lm_ctx_gather_kernel(const float* __restrict__ x, const int32_t* __restrict__ tokens, const LmCtxSeqs seqs,
                                                            const float* __restrict__ last, int ignore_index, float* __restrict__ hsel,
                                                            int32_t* __restrict__ targets) {
    int r = blockIdx.x, n = 0;
    for (; n < seqs.n; ++n) {
        if (!(seqs.flags[n] & kLmCtxScore)) continue;
        if (r < seqs.len[n]) break;
        r -= seqs.len[n];
    }
    if (n >= seqs.n) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    int tgt = ignore_index;  // token 0 on an empty slot: nothing predicts it
    if (r > 0) {
        v = reinterpret_cast<const f32x4*>(x + (long)(seqs.row0[n] + r - 1) * kHidden)[threadIdx.x];
        tgt = tokens[(long)seqs.tok0[n] + r];
    } else if (seqs.P[n] > 0) {
        v = reinterpret_cast<const f32x4*>(last + (long)seqs.slot[n] * kHidden)[threadIdx.x];
        tgt = tokens[(long)seqs.tok0[n]];
    }
    reinterpret_cast<f32x4*>(hsel + (long)blockIdx.x * kHidden)[threadIdx.x] = v;
    if (threadIdx.x == 0) targets[blockIdx.x] = tgt;
}

__global__ __launch_bounds__(192) void lm_ctx_last_kernel(const float* __restrict__ x, const LmCtxSeqs seqs, float* __restrict__ last) {
    const int n = blockIdx.x;
    if (!(seqs.flags[n] & kLmCtxCommit)) return;
    reinterpret_cast<f32x4*>(last + (long)seqs.slot[n] * kHidden)[threadIdx.x] =
        reinterpret_cast<const f32x4*>(x + (long)(seqs.row0[n] + seqs.len[n] - 1) * kHidden)[threadIdx.x];
}

bool lm_ctx_seqs_ok(const LmCtxSeqs& s) {
    if (s.n < 1 || s.n > kLmCtxMaxSeqs) return false;
    for (int n = 0; n < s.n; ++n)
        if (s.len[n] < 1 || s.P[n] < 0 || s.slot[n] < 0 || s.row0[n] < 0) return false;
    return true;
}

int lm_ctx_rows(const LmCtxSeqs& s) { return s.row0[s.n - 1] + s.len[s.n - 1]; }

}  // namespace

hipError_t launch_lm_ctx_attention(const float* qkv, const float* kcache, const float* vcache, long slot_stride, const LmCtxSeqs& seqs, float* out,
                                   hipStream_t s) {
    if (!qkv || !kcache || !vcache || !out || !lm_ctx_seqs_ok(seqs)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(kcache) | reinterpret_cast<uintptr_t>(vcache) | reinterpret_cast<uintptr_t>(out)) & 15)
        return hipErrorInvalidValue;
    if (slot_stride & 3) return hipErrorInvalidValue;
    int longest = 0;
    for (int n = 0; n < seqs.n; ++n) longest = seqs.len[n] > longest ? seqs.len[n] : longest;
    const int qtiles = (longest + LC_BQ - 1) / LC_BQ;
    hipLaunchKernelGGL(lm_ctx_attention_kernel, dim3((unsigned)(qtiles * kHeads), (unsigned)seqs.n), dim3(256), 0, s, qkv, kcache, vcache, slot_stride,
                       seqs, out);
    return hipGetLastError();
}

hipError_t launch_lm_ctx_embed(const int32_t* tokens, const LmCtxSeqs& seqs, const float* wte, int V, const float* wpe, float* x, int32_t* status,
                               hipStream_t s) {
    if (!tokens || !wte || !wpe || !x || V <= 0 || !lm_ctx_seqs_ok(seqs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_ctx_embed_kernel, dim3((unsigned)lm_ctx_rows(seqs)), dim3(192), 0, s, tokens, seqs, wte, V, wpe, x, status);
    return hipGetLastError();
}

hipError_t launch_lm_ctx_append(const float* qkv, const LmCtxSeqs& seqs, float* kcache, float* vcache, long slot_stride, hipStream_t s) {
    if (!qkv || !kcache || !vcache || !lm_ctx_seqs_ok(seqs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_ctx_append_kernel, dim3((unsigned)lm_ctx_rows(seqs)), dim3(384), 0, s, qkv, seqs, kcache, vcache, slot_stride);
    return hipGetLastError();
}

hipError_t launch_lm_ctx_gather(const float* x, const int32_t* tokens, const LmCtxSeqs& seqs, const float* last, int R, int ignore_index, float* hsel,
                                int32_t* targets, hipStream_t s) {
    if (!x || !tokens || !last || !hsel || !targets || R <= 0 || !lm_ctx_seqs_ok(seqs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_ctx_gather_kernel, dim3((unsigned)R), dim3(192), 0, s, x, tokens, seqs, last, ignore_index, hsel, targets);
    return hipGetLastError();
}

hipError_t launch_lm_ctx_last(const float* x, const LmCtxSeqs& seqs, float* last, hipStream_t s) {
    if (!x || !last || !lm_ctx_seqs_ok(seqs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_ctx_last_kernel, dim3((unsigned)seqs.n), dim3(192), 0, s, x, seqs, last);
    return hipGetLastError();
}

}  // namespace loco
