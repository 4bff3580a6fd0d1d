// Embedding neighbours: which rows of K [N, 768] are closest to each row of Q [M, 768], without ever forming the M x N score matrix.
//
//   row_norm2     n2[r] = sum_d x[r][d]^2 in double, rounded to fp32 once (one wave per row, one written order)
//   topk          the k best keys of every query under dot / cosine / l2 (the negated squared distance), best first, ties towards the
//                 lower key index; NaN scores, the query's `exclude` entry and keys >= N are not candidates; short lists end in (-inf, -1)
//   group_mean    out[g] = mean of rows[index[j]] over j in [offsets[g], offsets[g + 1]), sums in double: mean pooling of the ragged
//                 embedding store (index null, offsets the store's) and the k-means centre update (index = points sorted by label)
//
// ---- topk -------------------------------------------------------------------------------------------------------------------------
// The shape is lm.hip's lm_head_nll with a selection in place of the softmax.  A workgroup owns 128 queries and one CHUNK of
// kTopkChunk = 1024 keys.  It walks the chunk in tiles of 128 keys; each tile is the 128 x 128 x 768 exact-fp32 product of
// lm_head_partial_kernel (v_mfma_f32_32x32x2_f32, D = K_tile * Q_tile^T, operands through two XOR-swizzled LDS buffers, one barrier per
// k-tile, the running block sum folded every four k-tiles).  After a tile's k-loop the staging buffers are idle: the 128 x 128 scores
// -- scaled by the lanes that hold the dot products -- go into them key-major, and one thread per query scans its 128 scores in
// ascending key order against the query's running k-th best, inserting into a sorted (value, index) list kept in LDS (no per-lane array: the library's kernels use no private scratch).
// The next tile's first operands are fetched into registers before the scan, so the scan hides their latency.  After the chunk one
// record of k pairs per (query, chunk) is written; topk_merge_kernel folds a query's records in ascending chunk order by the same rule.
//
// The promise (lm.hip and decoder_score.hip make the same one): a query's k results are a function of the query's 768 values, its
// exclude entry, its norm and the keys alone, bit for bit -- not of M, of the query's row, of the slab it fell into or of its neighbours.
//   * a score is one MFMA chain over the 768 products in the order the tile walk fixes, whatever the query's slot in the tile, scaled
//     by one written expression;
//   * tile and chunk boundaries are multiples of 128 from key 0, so which keys meet in a list does not depend on M;
//   * candidates are offered in ascending key order and a candidate moves ahead of strictly smaller values only: (value desc, index asc);
//   * the merge walks the chunks in ascending order with that same rule.
// Keys >= N and queries >= M are never read: their addresses are clamped to the last valid row; clamped keys are not offered, clamped
// queries are not scanned and not written.
#include <math.h>

#include "loco_kernels.h"

namespace loco {

namespace {

constexpr int kNbTM = 128, kNbTN = 128, kNbBK = 32;
constexpr int kNbThreads = 256;
constexpr int kNbKTiles = kHidden / kNbBK;              // 24
constexpr int kNbTilesPerChunk = kTopkChunk / kNbTN;    // 8

// One candidate against a sorted list of `cnt` entries (capacity k) whose entry p lies at lv[p * stride], li[p * stride]; `kth` is the
// list's last value once it is full.  A candidate moves ahead of strictly smaller values only, so among equal values the one offered
// first -- the lower key index, as candidates come in ascending index order -- stays ahead.
__device__ __forceinline__ void topk_offer(float* lv, int* li, int stride, int k, int& cnt, float& kth, float s, int idx) {
    if (cnt == k && !(s > kth)) return;
    int p = cnt < k ? cnt : k - 1;
    while (p > 0 && lv[(p - 1) * stride] < s) {
        lv[p * stride] = lv[(p - 1) * stride];
        li[p * stride] = li[(p - 1) * stride];
        --p;
    }
    lv[p * stride] = s;
    li[p * stride] = idx;
    if (cnt < k) ++cnt;
    if (cnt == k) kth = lv[(k - 1) * stride];
}

// inv = 1 / max(sqrt(norm2), 1e-12): torch.nn.functional.normalize's eps
__device__ __forceinline__ float topk_inv_norm(float n2) { return 1.0f / fmaxf(sqrtf(n2), 1e-12f); }

__device__ __forceinline__ float topk_score(int metric, float dot, float qs, float ks) {
    if (metric == kTopkCosine) return (dot * qs) * ks;   // qs, ks: the inverse norms
    if (metric == kTopkL2) return (2.0f * dot - ks) - qs;  // qs, ks: the squared norms; 2 dot is exact, so a fused form rounds the same
    return dot;
}

__global__ __launch_bounds__(kNbThreads, 2) void topk_partial_kernel(const float* __restrict__ Q, long ldq, const float* __restrict__ K, long ldk,
                                                                    const float* __restrict__ qn2, const float* __restrict__ kn2,
                                                                    const int32_t* __restrict__ exclude, int M, int N, int k, int metric,
                                                                    int tiles_m, int nchunk, float* __restrict__ rec_v,
                                                                    int32_t* __restrict__ rec_i) {
    __shared__ __attribute__((aligned(16))) float lds[2][(kNbTM + kNbTN) * kNbBK];  // 64 KiB: operand staging, then the tile's scores
    __shared__ float list_v[kTopkMaxK * kNbTM];                                      // entry p of query row t at [p * 128 + t]
    __shared__ int list_i[kTopkMaxK * kNbTM];

    // query tile fastest: the workgroups that run together share one 3 MiB chunk of the keys
    const int rt = blockIdx.x % tiles_m, chunk = blockIdx.x / tiles_m;
    const int m0 = rt * kNbTM, c0 = chunk * kTopkChunk;
    const int ntile = min(kNbTilesPerChunk, (N - c0 + kNbTN - 1) / kNbTN);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    // staging, as lm_head_partial_kernel: thread -> rows tid / 8 + 32 j of the Q tile and of the K tile, 16-byte piece tid % 8 of the
    // row's 32 k, stored at piece ^ swz(row)
    const int srow = tid >> 3, spiece = tid & 7;
    int ga[4];  // floats from the tile's first query (ldq < 2^23: 128 rows stay inside 32 bits)
    int sdst[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = srow + 32 * j;
        const int gr = m0 + row < M ? m0 + row : M - 1;
        ga[j] = (gr - m0) * (int)ldq + 4 * spiece;
        const int swz = (((row >> 3) & 3) << 1) | ((row >> 1) & 1);
        sdst[j] = row * kNbBK + 4 * (spiece ^ swz);
    }
    const float* const Qm = Q + (long)m0 * ldq;
    f32x4 sa[4], sw[4];
    auto gload = [&](int tile, int kt) {
        const int n0 = c0 + tile * kNbTN;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = srow + 32 * j;
            const int gn = n0 + row < N ? n0 + row : N - 1;
            sa[j] = *reinterpret_cast<const f32x4*>(Qm + ga[j] + kt * kNbBK);
            sw[j] = *reinterpret_cast<const f32x4*>(K + (long)gn * ldk + 4 * spiece + kt * kNbBK);
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<f32x4*>(&lds[buf][sdst[j]]) = sa[j];
            *reinterpret_cast<f32x4*>(&lds[buf][kNbTM * kNbBK + sdst[j]]) = sw[j];
        }
    };

    const int fswz = (((r >> 3) & 3) << 1) | ((r >> 1) & 1);
    const int fa = (wm * 64 + r) * kNbBK;
    const int fw = (kNbTM + wn * 64 + r) * kNbBK;
    int fq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) fq[q] = 4 * ((4 * h + q) ^ fswz);

    // the scan's state: thread t < 128 owns query m0 + t
    const int qrow = m0 + tid;
    const bool scans = tid < kNbTM && qrow < M;
    int cnt = 0;
    float kth = 0.f;
    int excl = -1;
    if (scans && exclude) excl = exclude[qrow];
    float* const sc = &lds[0][0];  // the tile's scores, key-major: [key in tile][query in tile]

    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; tot[i][j][e] = 0.f; }

    gload(0, 0);
    for (int tile = 0; tile < ntile; ++tile) {
        sstore(0);
        __syncthreads();
        int cur = 0;
        for (int kt = 0; kt < kNbKTiles; ++kt) {
            const bool last_k = kt + 1 == kNbKTiles;
            if (!last_k) gload(tile, kt + 1);
            const float* lb = lds[cur];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(lb + fa + fq[q]);
                const f32x4 a1 = *reinterpret_cast<const f32x4*>(lb + fa + 32 * kNbBK + fq[q]);
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(lb + fw + fq[q]);
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(lb + fw + 32 * kNbBK + fq[q]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[e], a0[e], acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[e], a0[e], acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[e], a1[e], acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[e], a1[e], acc[1][1], 0, 0, 0);
                }
            }
            if (!last_k) sstore(cur ^ 1);
            __syncthreads();
            cur ^= 1;
            if (((kt + 1) & 3) == 0 && !last_k) {  // blocked accumulation, as gemm_f32.hip
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
        // The k-loop's last barrier has retired every read of the staging buffers.  acc[i][j][e] is query 64 wm + 32 i + r, key
        // 64 wn + 32 j + 8 (e >> 2) + 4 h + (e & 3) of the tile.  The lanes that hold the dot products scale them (one written expression,
        // topk_score); both norms are fetched here, the keys' four at a time: the register file is full during the k-loop.
        const int n0 = c0 + tile * kNbTN;
        int kbase = wn * 64 + 4 * h, rbase = wm * 64 + r;
        asm volatile("" : "+v"(kbase), "+v"(rbase));  // opaque: the addresses below, hoisted out of the k-loop, spilled to scratch
        float qs[2] = {0.f, 0.f};
        if (metric != kTopkDot) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float n2 = qn2[min(m0 + rbase + 32 * i, M - 1)];
                qs[i] = metric == kTopkCosine ? topk_inv_norm(n2) : n2;
            }
        }
#pragma unroll
        for (int jq = 0; jq < 8; ++jq) {  // four consecutive keys at a time: 64 wn + 32 j + 8 q + 4 h + {0 .. 3}
            const int j = jq >> 2, q = jq & 3;
            const int key0 = kbase + 32 * j + 8 * q;
            float ks[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ks[u] = 0.f;
                if (metric != kTopkDot) {
                    const float n2 = kn2[min(n0 + key0 + u, N - 1)];
                    ks[u] = metric == kTopkCosine ? topk_inv_norm(n2) : n2;
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = 4 * q + u;
                    sc[(key0 + u) * kNbTM + rbase + 32 * i] = topk_score(metric, tot[i][j][e] + acc[i][j][e], qs[i], ks[u]);
                    acc[i][j][e] = 0.f;
                    tot[i][j][e] = 0.f;
                }
        }
        if (tile + 1 < ntile) gload(tile + 1, 0);  // the next tile's first operands travel while the scan runs
        __syncthreads();
        if (scans) {
            // four scores at a time into registers, then each against the list: keys >= N, the excluded key and NaN are not offered
            for (int c = 0; c < kNbTN && n0 + c < N; c += 4) {
                float s[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] = sc[(c + u) * kNbTM + tid];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int key = n0 + c + u;
                    if (key < N && key != excl && s[u] == s[u]) topk_offer(list_v + tid, list_i + tid, kNbTM, k, cnt, kth, s[u], key);
                }
            }
        }
        __syncthreads();
    }

    if (scans) {
        const long base = ((long)qrow * nchunk + chunk) * k;
        for (int p = 0; p < k; ++p) {
            rec_v[base + p] = p < cnt ? list_v[p * kNbTM + tid] : -INFINITY;
            rec_i[base + p] = p < cnt ? list_i[p * kNbTM + tid] : -1;
        }
    }
}

// A query's records in ascending chunk order through topk_offer.  A record is sorted, so its first entry that the full list refuses ends it.
__global__ __launch_bounds__(64) void topk_merge_kernel(const float* __restrict__ rec_v, const int32_t* __restrict__ rec_i, int M, int k,
                                                        int nchunk, float* __restrict__ values, int32_t* __restrict__ indices) {
    __shared__ float list_v[kTopkMaxK * 64];
    __shared__ int list_i[kTopkMaxK * 64];
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * 64 + tid;
    if (row >= M) return;
    int cnt = 0;
    float kth = 0.f;
    for (int c = 0; c < nchunk; ++c) {
        const long base = (row * nchunk + c) * k;
        for (int p = 0; p < k; ++p) {
            const int idx = rec_i[base + p];
            if (idx < 0) break;
            const float s = rec_v[base + p];
            if (cnt == k && !(s > kth)) break;
            topk_offer(list_v + tid, list_i + tid, 64, k, cnt, kth, s, idx);
        }
    }
    for (int p = 0; p < k; ++p) {
        values[row * k + p] = p < cnt ? list_v[p * 64 + tid] : -INFINITY;
        indices[row * k + p] = p < cnt ? list_i[p * 64 + tid] : -1;
    }
}

// lane l sums elements l, l + 64, ... of its row ascending, in double; then wave_sum's butterfly; one rounding to fp32
__global__ __launch_bounds__(256) void row_norm2_kernel(const float* __restrict__ x, long ldx, long rows, float* __restrict__ n2) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;  // whole waves leave: wave_sum below stays inside one wave
    const int lane = threadIdx.x & 63;
    const float* p = x + row * ldx;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kHidden / 64; ++j) s += (double)p[lane + 64 * j] * (double)p[lane + 64 * j];
    s = wave_sum(s);
    if (lane == 0) n2[row] = (float)s;
}

// One workgroup per group: thread (p, c) = (tid / 192, tid % 192) sums columns 4 c .. 4 c + 3 of the group's rows j = p, p + 4, ...
// ascending, in double; the four partial sums meet in the order p = 0, 1, 2, 3.  The order depends on the group's size alone.
constexpr int kGmLanes = kHidden / 4;  // 192
constexpr int kGmPar = 4;
__global__ __launch_bounds__(kGmLanes * kGmPar) void group_mean_kernel(const float* __restrict__ rows, long ld, long n_rows,
                                                                     const int32_t* __restrict__ index, const int64_t* __restrict__ offsets,
                                                                     float* __restrict__ out, long ldo, int32_t* __restrict__ count) {
    __shared__ double part[kGmPar - 1][kHidden];
    __shared__ int bad_any;
    const long g = blockIdx.x;
    const long a = offsets[g], b = offsets[g + 1];
    const long n = b - a;
    const int tid = threadIdx.x, p = tid / kGmLanes, c = tid % kGmLanes;
    if (n <= 0) {  // an empty group: its row stays as it is
        if (tid == 0 && count) count[g] = 0;
        return;
    }
    if (tid == 0) bad_any = 0;
    __syncthreads();
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    bool bad = false;
    for (long j = a + p; j < b; j += kGmPar) {
        const long src = index ? (long)index[j] : j;
        if (src < 0 || src >= n_rows) { bad = true; continue; }  // never read; the group's mean becomes NaN
        const f32x4 v = *reinterpret_cast<const f32x4*>(rows + src * ld + 4 * c);
        s0 += (double)v[0]; s1 += (double)v[1]; s2 += (double)v[2]; s3 += (double)v[3];
    }
    if (bad) bad_any = 1;
    if (p > 0) {
        double* q = &part[p - 1][4 * c];
        q[0] = s0; q[1] = s1; q[2] = s2; q[3] = s3;
    }
    __syncthreads();
    if (p == 0) {
#pragma unroll
        for (int o = 0; o < kGmPar - 1; ++o) {
            const double* q = &part[o][4 * c];
            s0 += q[0]; s1 += q[1]; s2 += q[2]; s3 += q[3];
        }
        const double dn = (double)n;
        f32x4 m = {(float)(s0 / dn), (float)(s1 / dn), (float)(s2 / dn), (float)(s3 / dn)};
        if (bad_any) m = f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        *reinterpret_cast<f32x4*>(out + g * ldo + 4 * c) = m;
        if (tid == 0 && count) count[g] = (int32_t)(n > 0x7fffffffL ? 0x7fffffffL : n);
    }
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

long topk_chunks(long N) { return (N + kTopkChunk - 1) / kTopkChunk; }

size_t topk_scratch_bytes(long M, long N, int k) {
    if (M <= 0 || N <= 0 || N > 0x7fffffffL || M > 0x7fffffffL || k < 1 || k > kTopkMaxK) return 0;
    return (size_t)M * (size_t)topk_chunks(N) * (size_t)k * 8;
}

hipError_t launch_row_norm2(const float* x, long ldx, long rows, float* n2, hipStream_t s) {
    if (!x || !n2 || rows <= 0 || ldx < kHidden || (rows + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(row_norm2_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, ldx, rows, n2);
    return hipGetLastError();
}

hipError_t launch_topk(const float* Q, long ldq, const float* K, long ldk, const float* qn2, const float* kn2, const int32_t* exclude, long M,
                       long N, int k, int metric, float* values, int32_t* indices, void* scratch, hipStream_t s) {
    if (!Q || !K || !values || !indices || !scratch || M <= 0 || N <= 0 || k < 1 || k > kTopkMaxK) return hipErrorInvalidValue;
    if (metric != kTopkDot && metric != kTopkCosine && metric != kTopkL2) return hipErrorInvalidValue;
    if (metric != kTopkDot && (!qn2 || !kn2)) return hipErrorInvalidValue;
    if ((ldq | ldk) & 3 || ldq < kHidden || ldk < kHidden || ldq >= (1L << 23)) return hipErrorInvalidValue;
    if (misaligned16(Q) || misaligned16(K) || misaligned16(scratch)) return hipErrorInvalidValue;
    const long nchunk = topk_chunks(N);
    const long tiles_m = (M + kNbTM - 1) / kNbTM;
    if (M > 0x7fffffffL || N > 0x7fffffffL || tiles_m * nchunk > 0x7fffffffL) return hipErrorInvalidValue;
    float* rec_v = static_cast<float*>(scratch);
    int32_t* rec_i = reinterpret_cast<int32_t*>(rec_v + (size_t)M * nchunk * k);
    hipLaunchKernelGGL(topk_partial_kernel, dim3((unsigned)(tiles_m * nchunk)), dim3(kNbThreads), 0, s, Q, ldq, K, ldk, qn2, kn2, exclude, (int)M,
                       (int)N, k, metric, (int)tiles_m, (int)nchunk, rec_v, rec_i);
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, s, rec_v, rec_i, (int)M, k, (int)nchunk, values, indices);
    return hipGetLastError();
}

hipError_t launch_group_mean(const float* rows, long ld, long n_rows, const int32_t* index, const int64_t* offsets, long G, float* out, long ldo,
                             int32_t* count, hipStream_t s) {
    if (!rows || !offsets || !out || G <= 0 || G > 0x7fffffffL || n_rows <= 0) return hipErrorInvalidValue;
    if ((ld | ldo) & 3 || ld < kHidden || ldo < kHidden || misaligned16(rows) || misaligned16(out)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_mean_kernel, dim3((unsigned)G), dim3(kGmLanes * kGmPar), 0, s, rows, ld, n_rows, index, offsets, out, ldo, count);
    return hipGetLastError();
}

}  // namespace loco
