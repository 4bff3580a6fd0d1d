// GPT-2 language-model scorer: the kernels the encoder / decoder path did not have.
//
//   lm_head_nll   nll[r] = logsumexp_v(h[r] . wte[v]) - h[r] . wte[t[r]] over v < V, the [R, V] logits never stored
//   lm_embed      x[b,s,:] = wte[tokens[start[b] + s]] + wpe[s], ids read where they lie on the device
//   lm_gather     the rows that are scored, and their targets, out of the [B, S] body output
//   lm_transpose  HF Conv1D weights [in, out] -> the GEMM's [N, K] (once, at finalize)
// The layer body runs on launch_gemm (kEpiGeluNew is gemm_f32.hip's), launch_layernorm and launch_dec_attention.
//
// ---- lm_head_nll ------------------------------------------------------------------------------------------------------------
// A 50 257 x 768 product followed by a softmax: 31 % of GPT-2 base's FLOPs, and 2.6 GB of fp32 logits for one batch of 128 x 100
// tokens if they were written.  Here a workgroup owns 128 rows and one CHUNK of kLmChunk = 1024 vocabulary columns.  It walks the
// chunk in tiles of 128 columns; each tile is gemm_f32.hip's 128 x 128 x 768 product (v_mfma_f32_32x32x2_f32, D = W_tile * A_tile^T,
// operands staged through two XOR-swizzled LDS buffers, one barrier per k-tile, the running block sum folded every four k-tiles), and
// the tile's logits go from the accumulators straight into a running (max, sum of exp, target logit) that every lane keeps for its two
// rows over the columns it owns.  After the chunk's last tile the four lanes that share a row (two lane halves x two waves) meet in a
// fixed order and one (max, sum, target logit, found) record per (row, chunk) is written.  lm_head_merge_kernel then folds a row's
// records in ascending chunk order, in double.
//
// The promise (decoder_score.hip makes the same one): a row's nll is a function of the row's 768 values, its target and the weights
// alone, bit for bit -- not of R nor of where the row stands in the launch.
//   * a logit is one MFMA chain over k in the order the tile walk fixes, whatever the row's slot in the tile;
//   * which lane sums which column depends on the column's index only (chunk and tile boundaries are multiples of 128 from column 0);
//   * the per-lane sums, the lane-half step, the wave step and the chunk merge each have one written order.
// Columns >= V and rows >= R are never read (their addresses are clamped to the last valid one; clamped columns enter as -inf,
// clamped rows are not written).  NaN in h reaches nll through the sum (fmaxf drops NaN from the maxima, exp2 does not); +inf logits
// give inf - inf = NaN.
#include <math.h>

#include "loco_kernels.h"

namespace loco {

namespace {

constexpr int kLmTM = 128, kLmTN = 128, kLmBK = 32;
constexpr int kLmThreads = 256;
constexpr int kLmKTiles = kHidden / kLmBK;        // 24
constexpr int kLmTilesPerChunk = kLmChunk / kLmTN;  // 8
constexpr float kLmLog2e = 1.44269504088896340736f;

// (m, s) then (m2, s2), in that operand order: s = sum of exp(x - m) over the columns seen.  An empty side is (-inf, 0); the stand-in
// maximum 0 keeps -inf - -inf out of the exponent while a NaN sum still comes through (NaN * 0).
__device__ __forceinline__ void lm_merge2(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    const float mu = mn == -INFINITY ? 0.f : mn;
    s = s * __builtin_amdgcn_exp2f((m - mu) * kLmLog2e) + s2 * __builtin_amdgcn_exp2f((m2 - mu) * kLmLog2e);
    m = mn;
}

__global__ __launch_bounds__(kLmThreads, 2) void lm_head_partial_kernel(const float* __restrict__ H, long ldh, const float* __restrict__ W,
                                                                       long ldw, const int32_t* __restrict__ targets, int R, int V,
                                                                       int tiles_m, int nchunk, f32x4* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float lds[2][(kLmTM + kLmTN) * kLmBK];  // 64 KiB

    // row tile fastest: the workgroups that run together share one 3 MiB chunk of the weights
    const int rt = blockIdx.x % tiles_m, chunk = blockIdx.x / tiles_m;
    const int m0 = rt * kLmTM, c0 = chunk * kLmChunk;
    const int ntile = min(kLmTilesPerChunk, (V - c0 + kLmTN - 1) / kLmTN);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    // staging: thread -> rows tid / 8 + 32 j (j = 0..3) of the A tile and of the W tile, 16-byte piece tid % 8 of the row's 32 k;
    // stored at piece ^ swz(row), swz = {row bit 4, row bit 3, row bit 1} (gemm_f32.hip's swizzle: the fragment reads below are then
    // conflict-free)
    const int srow = tid >> 3, spiece = tid & 7;
    int ga[4];  // floats from the tile's first row (ldh < 2^23: 128 rows stay inside 32 bits)
    int sdst[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = srow + 32 * j;
        const int gr = m0 + row < R ? m0 + row : R - 1;
        ga[j] = (gr - m0) * (int)ldh + 4 * spiece;
        const int swz = (((row >> 3) & 3) << 1) | ((row >> 1) & 1);
        sdst[j] = row * kLmBK + 4 * (spiece ^ swz);
    }
    const float* const Hm = H + (long)m0 * ldh;
    f32x4 sa[4], sw[4];
    auto gload = [&](int tile, int kt) {
        const int n0 = c0 + tile * kLmTN;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = srow + 32 * j;
            const int gn = n0 + row < V ? n0 + row : V - 1;
            sa[j] = *reinterpret_cast<const f32x4*>(Hm + ga[j] + kt * kLmBK);
            sw[j] = *reinterpret_cast<const f32x4*>(W + (long)gn * ldw + 4 * spiece + kt * kLmBK);
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<f32x4*>(&lds[buf][sdst[j]]) = sa[j];
            *reinterpret_cast<f32x4*>(&lds[buf][kLmTM * kLmBK + sdst[j]]) = sw[j];
        }
    };

    // fragments: A rows 64 wm + {0, 32} + r, W rows 64 wn + {0, 32} + r; lane half h owns k [16 h, 16 h + 16) of the tile
    const int fswz = (((r >> 3) & 3) << 1) | ((r >> 1) & 1);
    const int fa = (wm * 64 + r) * kLmBK;
    const int fw = (kLmTM + wn * 64 + r) * kLmBK;
    int fq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) fq[q] = 4 * ((4 * h + q) ^ fswz);

    // this lane's two rows: 64 wm + 32 i + r
    int tgt[2];
    float run_m[2], run_s[2], run_t[2], run_f[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = m0 + wm * 64 + 32 * i + r;
        tgt[i] = row < R ? targets[row] : -1;
        run_m[i] = -INFINITY, run_s[i] = 0.f, run_t[i] = 0.f, run_f[i] = 0.f;
    }

    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; tot[i][j][e] = 0.f; }

    gload(0, 0);
    sstore(0);
    __syncthreads();

    int cur = 0;
    for (int tile = 0; tile < ntile; ++tile) {
        for (int kt = 0; kt < kLmKTiles; ++kt) {
            const bool last_k = kt + 1 == kLmKTiles;
            const bool more = !last_k || tile + 1 < ntile;
            if (more) gload(last_k ? tile + 1 : tile, last_k ? 0 : kt + 1);
            const float* lb = lds[cur];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(lb + fa + fq[q]);
                const f32x4 a1 = *reinterpret_cast<const f32x4*>(lb + fa + 32 * kLmBK + fq[q]);
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(lb + fw + fq[q]);
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(lb + fw + 32 * kLmBK + fq[q]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[e], a0[e], acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[e], a0[e], acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[e], a1[e], acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[e], a1[e], acc[1][1], 0, 0, 0);
                }
            }
            if (more) sstore(cur ^ 1);
            __syncthreads();
            cur ^= 1;
            if (((kt + 1) & 3) == 0 && !last_k) {  // blocked accumulation, as gemm_f32.hip: chains of 64 roundings, K / 128 block sums
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        tot[i][j] += acc[i][j];
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
                    }
            }
        }
        // The tile's logits: acc[i][j][e] is row 64 wm + 32 i + r, column n0 + 64 wn + 32 j + 8 (e >> 2) + 4 h + (e & 3).
        const int nb = c0 + tile * kLmTN + wn * 64 + 4 * h;
        const bool ragged = c0 + tile * kLmTN + kLmTN > V;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // two passes over the accumulators instead of a 32-register copy of the logits (the register file is full: no scratch)
            float tmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int col = nb + 32 * j + 8 * (e >> 2) + (e & 3);
                    float x = tot[i][j][e] + acc[i][j][e];
                    if (ragged && col >= V) x = -INFINITY;
                    if (col == tgt[i]) { run_t[i] = x; run_f[i] = 1.f; }
                    tmax = fmaxf(tmax, x);
                }
            const float mn = fmaxf(run_m[i], tmax);
            const float mu = mn == -INFINITY ? 0.f : mn;
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int col = nb + 32 * j + 8 * (e >> 2) + (e & 3);
                    float x = tot[i][j][e] + acc[i][j][e];
                    if (ragged && col >= V) x = -INFINITY;
                    sum += __builtin_amdgcn_exp2f((x - mu) * kLmLog2e);
                    acc[i][j][e] = 0.f;
                    tot[i][j][e] = 0.f;
                }
            run_s[i] = run_s[i] * __builtin_amdgcn_exp2f((run_m[i] - mu) * kLmLog2e) + sum;
            run_m[i] = mn;
        }
    }

    // the four lanes of a row: lane half 0 then 1, wave wn = 0 then 1.  The loop's last barrier has retired every LDS read.
    f32x4* xch = reinterpret_cast<f32x4*>(&lds[0][0]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float om = __shfl_xor(run_m[i], 32, 64), os = __shfl_xor(run_s[i], 32, 64);
        const float ot = __shfl_xor(run_t[i], 32, 64), of = __shfl_xor(run_f[i], 32, 64);
        float m = h ? om : run_m[i], s = h ? os : run_s[i];
        lm_merge2(m, s, h ? run_m[i] : om, h ? run_s[i] : os);
        const float t = run_f[i] != 0.f ? run_t[i] : ot, f = fmaxf(run_f[i], of);
        run_m[i] = m, run_s[i] = s, run_t[i] = t, run_f[i] = f;
        if (wn == 1 && h == 0) xch[wm * 64 + 32 * i + r] = f32x4{m, s, t, f};
    }
    __syncthreads();
    if (wn == 0 && h == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = m0 + wm * 64 + 32 * i + r;
            if (row >= R) continue;
            const f32x4 o = xch[wm * 64 + 32 * i + r];
            float m = run_m[i], s = run_s[i];
            lm_merge2(m, s, o[0], o[1]);
            part[(long)row * nchunk + chunk] = f32x4{m, s, run_f[i] != 0.f ? run_t[i] : o[2], fmaxf(run_f[i], o[3])};
        }
    }
}

// nll[r] from the row's records, ascending chunk order, in double: (M - target logit) + log(sum_c s_c exp(m_c - M))
__global__ __launch_bounds__(256) void lm_head_merge_kernel(const f32x4* __restrict__ part, const int32_t* __restrict__ targets, int R, int V,
                                                            int nchunk, int ignore_index, float* __restrict__ nll) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= R) return;
    const int t = targets[row];
    if (t == ignore_index) { nll[row] = 0.f; return; }
    if (t < 0 || t >= V) { nll[row] = __builtin_nanf(""); return; }
    const f32x4* p = part + (long)row * nchunk;
    float M = -INFINITY;
    for (int c = 0; c < nchunk; ++c) M = fmaxf(M, p[c][0]);
    double S = 0.0, tl = 0.0;
    for (int c = 0; c < nchunk; ++c) {
        const f32x4 q = p[c];
        S += (double)q[1] * (q[0] == -INFINITY ? 0.0 : exp((double)q[0] - (double)M));
        if (q[3] != 0.f) tl = (double)q[2];
    }
    nll[row] = (float)(((double)M - tl) + log(S));
}

__global__ __launch_bounds__(192) void lm_embed_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ start,
                                                       const int32_t* __restrict__ len, const float* __restrict__ wte, int V,
                                                       const float* __restrict__ wpe, float* __restrict__ x, int S, int32_t* status) {
    const int s = blockIdx.x, b = blockIdx.y;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (s < len[b]) {
        const long pos = (long)start[b] + s;
        const int id = tokens[pos];
        if (id >= 0 && id < V) {
            v = reinterpret_cast<const f32x4*>(wte + (long)id * kHidden)[threadIdx.x] + reinterpret_cast<const f32x4*>(wpe + (long)s * kHidden)[threadIdx.x];
        } else if (threadIdx.x == 0 && status) {
            atomicMin(status, (int)min(pos, (long)0x7ffffffe));
        }
    }
    reinterpret_cast<f32x4*>(x + ((long)b * S + s) * kHidden)[threadIdx.x] = v;
}

__global__ __launch_bounds__(192) void lm_gather_kernel(const float* __restrict__ x, const int32_t* __restrict__ rows,
                                                        const int32_t* __restrict__ tokens, const int32_t* __restrict__ start,
                                                        const int32_t* __restrict__ len, int B, int S, int ignore_index, float* __restrict__ out,
                                                        int32_t* __restrict__ targets) {
    const int r = blockIdx.x;
    const int idx = rows[r];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    int t = -1;  // a row index outside [0, B S): no valid target, NaN
    if (idx >= 0 && idx < B * S) {
        const int b = idx / S, s = idx % S;
        v = reinterpret_cast<const f32x4*>(x + (long)idx * kHidden)[threadIdx.x];
        t = s + 1 < min(len[b], S) ? tokens[(long)start[b] + s + 1] : ignore_index;
    }
    reinterpret_cast<f32x4*>(out + (long)r * kHidden)[threadIdx.x] = v;
    if (threadIdx.x == 0) targets[r] = t;
}

// out[c][r] = in[r][c]
__global__ __launch_bounds__(256) void lm_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int cols) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < rows && c0 + tx < cols) tile[k][tx] = in[(long)(r0 + k) * cols + c0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (c0 + k < cols && r0 + tx < rows) out[(long)(c0 + k) * rows + r0 + tx] = tile[tx][k];
}

// mean of nll over each group's items, in double, ascending: group g owns items [offsets[g], offsets[g + 1])
__global__ __launch_bounds__(64) void lm_group_mean_kernel(const float* __restrict__ nll, const int32_t* __restrict__ offsets, int G,
                                                           double* __restrict__ mean, double* __restrict__ ppl) {
    const int g = blockIdx.x;
    const int a = offsets[g], b = offsets[g + 1];
    double s = 0.0;  // lane l sums items a + l, a + l + 64, ... ascending; then wave_sum's butterfly: an order that depends on (a, b) only
    for (int i = a + (int)threadIdx.x; i < b; i += 64) s += (double)nll[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        const double m = b > a ? s / (double)(b - a) : __builtin_nan("");
        mean[g] = m;
        ppl[g] = exp(m);
    }
}

}  // namespace

int lm_head_chunks(int V) { return (V + kLmChunk - 1) / kLmChunk; }
size_t lm_head_scratch_bytes(long R, int V) { return R > 0 && V > 0 ? (size_t)R * lm_head_chunks(V) * sizeof(f32x4) : 0; }

hipError_t launch_lm_head_nll(const float* h, long ldh, const float* wte, long ldw, const int32_t* targets, long R, int V, int ignore_index,
                              float* nll, void* scratch, hipStream_t s) {
    if (!h || !wte || !targets || !nll || !scratch || R <= 0 || V <= 0) return hipErrorInvalidValue;
    if ((ldh | ldw) & 3 || ldh < kHidden || ldw < kHidden || ldh >= (1L << 23)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(wte) | reinterpret_cast<uintptr_t>(scratch)) & 15) return hipErrorInvalidValue;
    const int nchunk = lm_head_chunks(V);
    const long tiles_m = (R + kLmTM - 1) / kLmTM;
    if (R > 0x7fffffffL || tiles_m * nchunk > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_head_partial_kernel, dim3((unsigned)(tiles_m * nchunk)), dim3(kLmThreads), 0, s, h, ldh, wte, ldw, targets, (int)R, V,
                       (int)tiles_m, nchunk, static_cast<f32x4*>(scratch));
    hipLaunchKernelGGL(lm_head_merge_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, static_cast<const f32x4*>(scratch), targets, (int)R,
                       V, nchunk, ignore_index, nll);
    return hipGetLastError();
}

hipError_t launch_lm_embed(const int32_t* tokens, const int32_t* start, const int32_t* len, const float* wte, int V, const float* wpe, float* x,
                           int B, int S, int32_t* status, hipStream_t s) {
    if (!tokens || !start || !len || !wte || !wpe || !x || B <= 0 || S <= 0 || V <= 0 || B > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_embed_kernel, dim3((unsigned)S, (unsigned)B), dim3(192), 0, s, tokens, start, len, wte, V, wpe, x, S, status);
    return hipGetLastError();
}

hipError_t launch_lm_gather(const float* x, const int32_t* rows, const int32_t* tokens, const int32_t* start, const int32_t* len, int B, int S,
                            int R, int ignore_index, float* out, int32_t* targets, hipStream_t s) {
    if (!x || !rows || !tokens || !start || !len || !out || !targets || R <= 0 || (long)B * S > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_gather_kernel, dim3((unsigned)R), dim3(192), 0, s, x, rows, tokens, start, len, B, S, ignore_index, out, targets);
    return hipGetLastError();
}

hipError_t launch_lm_transpose(const float* in, float* out, int rows, int cols, hipStream_t s) {
    if (!in || !out || rows <= 0 || cols <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_transpose_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, s, in, out, rows, cols);
    return hipGetLastError();
}

hipError_t launch_lm_group_mean(const float* nll, const int32_t* offsets, int G, double* mean, double* ppl, hipStream_t s) {
    if (!nll || !offsets || !mean || !ppl || G <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_group_mean_kernel, dim3((unsigned)G), dim3(64), 0, s, nll, offsets, G, mean, ppl);
    return hipGetLastError();
}

}  // namespace loco
