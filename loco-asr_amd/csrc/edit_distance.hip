// Edit distance over int32 symbol sequences and the expected-distance risk of n-best lists (metrics.py: CER / WER, MBR selection).
//
// The rule (include/loco_asr.h, "error rates"): a cell is the pair (cost, S), compared lexicographically,
//   D[i][0] = (i, 0), D[0][j] = (j, 0), D[i][j] = min(D[i-1][j-1] + (a[i-1] == b[j-1] ? (0,0) : (1,1)), D[i-1][j] + (1,0), D[i][j-1] + (1,0)),
// packed as cost << 16 | S in one u32, so that ONE unsigned min is the lexicographic min.  Both fields stay below 65 536 because a side
// holds at most kEditMaxLen = 16 384 symbols (cost <= max(n, m), S <= min(n, m)).  The result is a property of the pair of sequences,
// not of a traceback order: minimum cost, then most correct symbols.
//
// edit_distance_kernel: ONE WAVE PER PAIR and no workgroup barrier anywhere -- the waves of a workgroup share nothing, finish at
// different times and leave.  The sweep is skewed and striped.  With b the shorter side (m symbols; the sides are swapped when the
// hypothesis is the longer one, and D and I with them, which the rule makes exact), lane l owns the c = ceil(m / 64) columns
// l*c + 1 .. (l+1)*c.  At step t it walks row i = t - l through its columns in order: the left neighbour of a cell is the cell the lane
// has just computed, the upper one is the lane's own row state, and only the first column looks outside the lane -- at D[i][l*c], the
// last cell lane l - 1 computed one step earlier (one __shfl_up of one u32 per step), and at D[i-1][l*c], the value received one step
// before that and kept.  Lane 0 reads the boundary (i, 0).  n + (active lanes) - 1 steps; the answer is the last cell of the lane
// that owns column m, after row n.
//
// Row state: LDS, in the layout [k * 64 + lane] (k = the column's index inside the lane's stripe): the 32 lanes a ds_read_b32 /
// ds_write_b32 serves together sit on 32 different banks, so there is no bank conflict, and a lane only ever touches its own
// entries, so there is nothing to synchronise.  A launch sizes the stripe by its own longest shorter side (`max_len`), not by the cap:
//   form A, max_len <= 2048 (c <= 32): 4 waves (pairs) per 256-thread workgroup; the lane's symbols of b sit in LDS beside its row
//           (2 * c * 256 B per wave, 64 KiB per workgroup at c = 32) -- every transcript-sized pair;
//   form B, up to the cap (c <= 256): one wave per workgroup with up to 64 KiB of row state, b read from memory (L1 / L2) as the
//           lane walks its stripe.  Four such pairs do not fit one workgroup's LDS.
// Registers for the row were the alternative for small c; the LDS form is one loop for every c, costs one ds_read and one ds_write
// per cell beside about eight VALU operations, and leaves the occupancy to the LDS a launch really needs (512 B per wave at c = 1).
#include <hip/hip_runtime.h>

#include "loco_kernels.h"

namespace loco {

namespace {

constexpr int kFormAMaxC = 32;  // 4 waves * 2 arrays * 32 * 256 B = 64 KiB

__device__ __forceinline__ void write_counts(int32_t* out, int s, int d, int i, int h) {
    out[0] = s; out[1] = d; out[2] = i; out[3] = h;
}

// cstride: the stripe a wave's LDS holds (columns per lane), >= the c of every pair the launch computes.
template <int WAVES, bool B_IN_LDS>
__global__ __launch_bounds__(WAVES * 64) void edit_distance_kernel(const int32_t* __restrict__ symbols, long n_symbols,
                                                                   const int32_t* __restrict__ spans, int P, int cstride,
                                                                   int32_t* __restrict__ counts) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long p = (long)blockIdx.x * WAVES + wave;
    if (p >= P) return;
    uint32_t* row = lds + (size_t)wave * (B_IN_LDS ? 2 : 1) * cstride * 64;
    uint32_t* bsym = row + (size_t)cstride * 64;  // form A only

    const int4 span = reinterpret_cast<const int4*>(spans)[p];  // 16-byte aligned: the entry refuses another pointer
    const int rs = span.x, rn = span.y, hs = span.z, hn = span.w;
    int32_t* out = counts + p * 4;
    const bool bad = rn < 0 || hn < 0 || rn > kEditMaxLen || hn > kEditMaxLen || rs < 0 || hs < 0 || (long)rs + rn > n_symbols ||
                     (long)hs + hn > n_symbols || min(rn, hn) > cstride * 64;
    if (bad) {  // nothing of the pair is read
        if (lane == 0) write_counts(out, -1, -1, -1, -1);
        return;
    }
    const bool swapped = hn > rn;  // b, the striped side, is the shorter one
    const int32_t* a = symbols + (swapped ? hs : rs);
    const int32_t* b = symbols + (swapped ? rs : hs);
    const int n = swapped ? hn : rn, m = swapped ? rn : hn;

    uint32_t last = (uint32_t)n << 16;  // m == 0: D[n][0] = (n, 0)
    int owner = 0;
    if (m > 0) {
        const int c = (m + 63) >> 6;
        const int active = (m + c - 1) / c;  // lanes that own a column
        owner = active - 1;
        const int col0 = lane * c;           // the lane's columns are col0 + 1 .. col0 + ncols
        const int ncols = min(max(m - col0, 0), c);
        for (int k = 0; k < ncols; ++k) {
            row[k * 64 + lane] = (uint32_t)(col0 + 1 + k) << 16;  // D[0][j] = (j, 0)
            if (B_IN_LDS) bsym[k * 64 + lane] = (uint32_t)b[col0 + k];
        }
        uint32_t corner = (uint32_t)col0 << 16;  // D[i-1][col0] of the row the lane computes next; row 1: D[0][col0]
        const int steps = n + active - 1;
        int32_t a_next = lane == 0 ? a[0] : 0;  // a[i-1] of the lane's row at the next step (n >= m >= 1)
        for (int t = 1; t <= steps; ++t) {
            const uint32_t recv = __shfl_up(last, 1);  // every lane takes part; lane l-1's last cell of step t-1 is D[t-l][col0]
            const int i = t - lane;
            const int32_t ai = a_next;
            const int inext = i + 1;  // fetched one step ahead of its use
            a_next = (lane < active && inext >= 1 && inext <= n) ? a[inext - 1] : 0;
            if (lane < active && i >= 1 && i <= n) {
                const uint32_t edge = lane == 0 ? (uint32_t)i << 16 : recv;  // D[i][col0]
                uint32_t left = edge, diag = corner;
                for (int k = 0; k < ncols; ++k) {
                    const uint32_t up = row[k * 64 + lane];
                    const int32_t bj = B_IN_LDS ? (int32_t)bsym[k * 64 + lane] : b[col0 + k];
                    const uint32_t cell = min(diag + (ai == bj ? 0u : 0x10001u), min(up, left) + 0x10000u);
                    row[k * 64 + lane] = cell;
                    diag = up;
                    left = cell;
                }
                last = left;
                corner = edge;
            }
        }
    }
    if (lane == owner) {
        const int cost = (int)(last >> 16), S = (int)(last & 0xffffu);
        const int del = (cost - S + n - m) / 2, ins = (cost - S - n + m) / 2;  // of a against b: D - I = n - m, D + I = cost - S
        write_counts(out, S, swapped ? ins : del, swapped ? del : ins, n - S - del);
    }
}

// One wave per group u of N = group_offsets[u + 1] - group_offsets[u] hypotheses; the group's pairs (i < j) lie row-major in `counts`
// behind the pairs of the groups before it.  risk[h] = (sum over h' != h, ascending, of w[h'] * cost(h, h')) / (sum over h', ascending,
// of w[h']) in double, products and sums rounded one by one (no fused multiply-add: the host restatement adds the same numbers).
__global__ __launch_bounds__(64) void nbest_risk_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ group_offsets,
                                                        const double* __restrict__ weights, int U, double* __restrict__ risk,
                                                        int32_t* __restrict__ best) {
#pragma clang fp contract(off)
    const int u = blockIdx.x, lane = threadIdx.x;
    if (u >= U) return;
    long before = 0;  // pairs of the groups before u: integers, any order
    for (int g = lane; g < u; g += 64) {
        const long N = group_offsets[g + 1] - group_offsets[g];
        before += N * (N - 1) / 2;
    }
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    const int h0 = group_offsets[u], N = group_offsets[u + 1] - h0;
    const int32_t* pc = counts + before * 4;
    double den = 0.0;
    for (int j = 0; j < N; ++j) den = den + (weights ? weights[h0 + j] : 1.0);
    double best_risk = 0.0;
    int best_h = 0x7fffffff;
    for (int h = lane; h < N; h += 64) {
        double num = 0.0;
        for (int j = 0; j < N; ++j) {
            if (j == h) continue;
            const long lo = min(h, j), hi = max(h, j);
            const int32_t* q = pc + (lo * N - lo * (lo + 1) / 2 + (hi - lo - 1)) * 4;
            const double cost = (double)(q[0] + q[1] + q[2]);
            const double term = (weights ? weights[h0 + j] : 1.0) * cost;
            num = num + term;
        }
        const double r = num / den;
        risk[h0 + h] = r;
        if (best_h == 0x7fffffff || r < best_risk) {  // ascending h: the first of equal risks stays
            best_risk = r;
            best_h = h;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double r = __shfl_xor(best_risk, off);
        const int h = __shfl_xor(best_h, off);
        if (h != 0x7fffffff && (best_h == 0x7fffffff || r < best_risk || (r == best_risk && h < best_h))) {
            best_risk = r;
            best_h = h;
        }
    }
    if (lane == 0) best[u] = N > 0 ? best_h : -1;
}

}  // namespace

hipError_t launch_edit_distance(const int32_t* symbols, long n_symbols, const int32_t* spans, int P, int max_len, int32_t* counts,
                                hipStream_t s) {
    if (P <= 0) return hipSuccess;
    const int c = max_len > 0 ? (max_len + 63) / 64 : 1;
    if (c <= kFormAMaxC) {
        constexpr int W = 4;
        const size_t lds = (size_t)W * 2 * c * 64 * sizeof(uint32_t);
        edit_distance_kernel<W, true><<<dim3((unsigned)((P + W - 1) / W)), dim3(W * 64), lds, s>>>(symbols, n_symbols, spans, P, c, counts);
    } else {
        const size_t lds = (size_t)c * 64 * sizeof(uint32_t);
        edit_distance_kernel<1, false><<<dim3((unsigned)P), dim3(64), lds, s>>>(symbols, n_symbols, spans, P, c, counts);
    }
    return hipGetLastError();
}

hipError_t launch_nbest_risk(const int32_t* counts, const int32_t* group_offsets, const double* weights, int U, double* risk, int32_t* best,
                             hipStream_t s) {
    if (U <= 0) return hipSuccess;
    nbest_risk_kernel<<<dim3((unsigned)U), dim3(64), 0, s>>>(counts, group_offsets, weights, U, risk, best);
    return hipGetLastError();
}

}  // namespace loco
