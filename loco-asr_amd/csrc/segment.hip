// Cutting a long recording into utterance-sized segments at pauses, on the device where the waveform lives after resampling
// (include/loco_asr.h "long-form segmentation").  There is no counterpart in the reference: the rules are this
// project's own, restated in numpy by tests/segment_ref.py, and every rule below that decides a frame, a run or a cut is integer or
// exact fp32 arithmetic, so that the two agree bit for bit on the same db array.
//
// Frames are the encoder's: frame t covers samples [320 t, 320 t + 400), F = loco_output_frames(n) = (n - 80) / 320.
//
// A recording has C channels with one speaker per channel (a two-channel telephone call); a mono recording is C = 1, the same kernels
// launched with one channel.  Every channel is cut on its own, by the same rules:
//   frame_energy_db_kernel   db[c][t] = 10 log10(mean(x^2) + 1e-12) for wav [C, stride]: the grid's y is the channel, one wave per frame,
//                            lane l squares samples l, l + 64, ... in that order with fmaf, the lanes meet in wave_sum -- a frame's bits
//                            do not depend on where it is computed.
//   vad_segments_kernel      ONE workgroup of 1024 threads per channel, the grid is C.  Parallel across the workgroup: the histogram (LDS
//                            integer atomics), the speech mask, the run boundaries (chunked count + block scan, three times: raw mask,
//                            gaps filled, short speech dropped) and each step's scan of its window.  Sequential: the walk over cuts, at
//                            most F / min(min_frames + 1, max_frames / 2) steps of two or three barriers each.  With C > 1 there is one
//                            addition, the cross-talk gate (restated by tests/segment_channels_ref.py; this project's own rule like the
//                            rest, its 15 dB default not validated on real calls): at the raw-mask step a frame is also required NOT to
//                            have another channel louder by more than crosstalk_db (the maximum over the other channels, NaN ignored;
//                            one fp32 subtraction, a strict >).  The threshold stays the channel's own, ungated.  The other rows of db
//                            are inputs only: no workgroup waits for another, and a one-channel launch (the kernel template's other
//                            instantiation, compiled without the gate) reads no other row.  The cleaned mask stays in the channel's
//                            workspace slice (all zero for a silent channel).
//   vad_overlap_kernel       a second launch, one wave per (channel, segment): the frames of the segment in which any other channel's
//                            cleaned mask is set.
// Channels are addressed by strides from one base pointer; there is no array of pointers in an argument struct.
// Memory: per channel F bytes of mask, F + 1 run boundaries and F run indices in the workspace (vad_layout; global, read back by other
// waves of the same workgroup only behind __syncthreads()).  Nothing here is larger than 180 000 frames x 9 bytes for an hour of audio.
#include <cmath>

#include "loco_kernels.h"

namespace loco {

namespace {
constexpr int kVadThreads = 1024;
constexpr int kVadWaves = kVadThreads / 64;
typedef unsigned long long u64;

// One frame's energy in dB, computed by one wave from the frame's 400 samples at x; the same value in every lane.
__device__ __forceinline__ float frame_energy_db_of(const float* __restrict__ x, int lane) {
    float acc = 0.f;
#pragma unroll
    for (int i = lane; i < kVadWindow; i += 64) acc = fmaf(x[i], x[i], acc);
    const float mean = wave_sum(acc) / (float)kVadWindow;
    // 10 log10(1e-12) is -120 exactly; log10f's last bit is not relied on for it
    return mean == 0.f ? -120.f : 10.f * log10f(mean + 1e-12f);
}

// wav [C, stride] -> db [C, F]; blockIdx.y = the channel
__global__ __launch_bounds__(256) void frame_energy_db_kernel(const float* __restrict__ wav, long stride, long F, float* __restrict__ db) {
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= F) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const float v = frame_energy_db_of(wav + (long)blockIdx.y * stride + t * kVadHop, lane);
    if (lane == 0) db[(long)blockIdx.y * F + t] = v;
}

// 0.25 dB bins from -120 dB: the scaling by 4 is exact, so no contraction can move a value across an edge.  NaN: bin 0.
__device__ __forceinline__ int vad_bin(float v) {
    if (!(v == v)) return 0;
    const float t = floorf((v - (-120.f)) * 4.f);
    return t < 0.f ? 0 : (t > (float)(kVadBins - 1) ? kVadBins - 1 : (int)t);
}

// floats in a total order as unsigned integers: NaN lowest, then -inf ... -0 < +0 ... +inf
__device__ __forceinline__ unsigned vad_order_key(float v) {
    if (!(v == v)) return 0u;
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// maximum of v over the workgroup, the same value in every thread; sh: kVadWaves words of LDS, free again on return
__device__ __forceinline__ u64 block_max_u64(u64 v, u64* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = sh[0];
#pragma unroll
    for (int i = 1; i < kVadWaves; ++i) r = sh[i] > r ? sh[i] : r;
    __syncthreads();
    return r;
}

// exclusive prefix sum of v over the workgroup's threads; *total = the sum, in every thread
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kVadWaves; ++i) {
        if (i < w) base += sh[i];
        tot += sh[i];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// Runs of equal mask values: bnd[r] = first frame of run r (bnd[R] = F), rid[t] = the run frame t lies in.  Returns R.  Thread i owns
// the frames [i chunk, (i + 1) chunk): it counts the runs that start there, the counts meet in one scan, it writes its frames.
// Ends with a barrier: bnd and rid are readable by every thread on return.
__device__ int build_runs(const unsigned char* mask, int F, int32_t* bnd, int32_t* rid, int* sh) {
    const int chunk = (F + kVadThreads - 1) / kVadThreads;
    const long c0l = (long)threadIdx.x * chunk;
    const int c0 = c0l < F ? (int)c0l : F, c1 = c0 + chunk < F ? c0 + chunk : F;
    int starts = 0;
    for (int t = c0; t < c1; ++t) starts += (t == 0 || mask[t] != mask[t - 1]) ? 1 : 0;
    int R;
    int cur = block_excl_scan(starts, sh, &R) - 1;  // the run frame c0 - 1 lies in
    for (int t = c0; t < c1; ++t) {
        if (t == 0 || mask[t] != mask[t - 1]) bnd[++cur] = t;
        rid[t] = cur;
    }
    if (threadIdx.x == 0) bnd[R] = F;
    __syncthreads();
    return R;
}

// The cross-talk gate of the channel kernel: frame t of channel c is not speech when another channel is louder there by more than
// crosstalk_db.  other = the maximum over the other channels with NaN ignored; no other value: not gated.  One fp32 subtraction and a
// strict >, so +inf switches the gate off and a difference of exactly crosstalk_db is kept.
__device__ __forceinline__ bool vad_crosstalk_gated(const float* __restrict__ dball, int C, int c, long F, int t, float v, float crosstalk_db) {
    bool any = false;
    float other = 0.f;
    for (int o = 0; o < C; ++o) {
        if (o == c) continue;
        const float u = dball[(long)o * F + t];
        if (u == u) {
            other = any ? (u > other ? u : other) : u;
            any = true;
        }
    }
    return any && (other - v > crosstalk_db);
}

// The rules of one channel, run by one workgroup of kVadThreads: channel ch = blockIdx.x owns row ch of dball [C, F], of seg_start /
// seg_end [C, max_segments], count [C] and thr_out [C], and the ch-th slice of the workspace (vad_layout: the mask at 0, bnd at
// bnd_off, rid at rid_off); the other rows of dball are read by the gate alone.  kMono is the C == 1 launch, compiled without the gate
// and with ch = 0 (as one kernel with a uniform `C > 1 &&` in front of the gate the one-channel launch measured about 1 % slower):
// it reads no other row and touches nothing beyond the one slice's vad_layout().bytes.  A silent channel leaves an all-zero mask
// behind, for vad_overlap_kernel -- with kMono too, where nothing reads it: F bytes of caller-provided scratch, no output depends on them.
template <bool kMono>
__global__ __launch_bounds__(kVadThreads) void vad_segments_kernel(const float* __restrict__ dball, int C, float crosstalk_db, VadArgs a,
                                                                    int32_t* __restrict__ seg_start, int32_t* __restrict__ seg_end,
                                                                    int32_t* __restrict__ count, float* __restrict__ thr_out, unsigned char* ws,
                                                                    long slice, long bnd_off, long rid_off) {
    __shared__ int hist[kVadBins];
    __shared__ int sh_i[kVadWaves];
    __shared__ u64 sh_q[kVadWaves];
    __shared__ int sh_mode;
    __shared__ float sh_thr;
    const int tid = threadIdx.x, F = a.F, ch = kMono ? 0 : blockIdx.x;
    const float* __restrict__ db = dball + (long)ch * F;
    unsigned char* mask = ws + (long)ch * slice;
    int32_t* bnd = reinterpret_cast<int32_t*>(mask + bnd_off);
    int32_t* rid = reinterpret_cast<int32_t*>(mask + rid_off);
    seg_start += (long)ch * a.max_segments;
    seg_end += (long)ch * a.max_segments;
    count += ch;
    thr_out += ch;

    // ---- threshold: the channel's own histogram, not gated ----
    for (int i = tid; i < kVadBins; i += kVadThreads) hist[i] = 0;
    __syncthreads();
    for (int t = tid; t < F; t += kVadThreads) atomicAdd(&hist[vad_bin(db[t])], 1);
    __syncthreads();
    if (tid == 0) {
        int cum = 0, nb = -1, pb = -1;
        for (int i = 0; i < kVadBins; ++i) {
            cum += hist[i];
            if (nb < 0 && cum >= a.k_noise) nb = i;
            if (pb < 0 && cum >= a.k_peak) pb = i;
        }
        const float noise = -120.f + 0.25f * (float)nb, peak = -120.f + 0.25f * (float)pb;  // exact
        int mode = kVadNormal;
        float thr = fmaxf(a.abs_floor_db, noise + a.margin_db);
        if (peak < a.abs_floor_db) {
            mode = kVadSilent;
            thr = INFINITY;
        } else if (peak - noise < a.min_dynamic_db) {
            mode = kVadAllSpeech;
            thr = -INFINITY;
        }
        sh_mode = mode;
        sh_thr = thr;
        *thr_out = thr;
        if (mode == kVadSilent) *count = 0;
    }
    __syncthreads();
    const int mode = sh_mode;
    const float thr = sh_thr;
    if (mode == kVadSilent) {  // uniform
        for (int t = tid; t < F; t += kVadThreads) mask[t] = 0;
        return;
    }

    // ---- mask and clean-up ----
    for (int t = tid; t < F; t += kVadThreads) {
        const float v = db[t];
        const bool base = mode == kVadAllSpeech ? v == v : v > thr;
        mask[t] = (base && !(!kMono && vad_crosstalk_gated(dball, C, ch, F, t, v, crosstalk_db))) ? 1 : 0;
    }
    __syncthreads();
    int R = build_runs(mask, F, bnd, rid, sh_i);
    int m0 = mask[0];
    for (int r = tid + 1; r < R - 1; r += kVadThreads) {  // interior silence runs shorter than min_silence become speech
        const int lo = bnd[r], hi = bnd[r + 1];
        if (((m0 ^ r) & 1) == 0 && hi - lo < a.min_silence)
            for (int t = lo; t < hi; ++t) mask[t] = 1;
    }
    __syncthreads();
    R = build_runs(mask, F, bnd, rid, sh_i);
    for (int r = tid; r < R; r += kVadThreads) {  // then speech runs shorter than min_speech become silence
        const int lo = bnd[r], hi = bnd[r + 1];
        if (((m0 ^ r) & 1) == 1 && hi - lo < a.min_speech)
            for (int t = lo; t < hi; ++t) mask[t] = 0;
    }
    __syncthreads();
    R = build_runs(mask, F, bnd, rid, sh_i);
    m0 = mask[0];

    // ---- the walk over cuts: s, c and n are the same in every thread ----
    int s = 0, n = 0;
    while (s < F) {
        int c = F;
        if (F - s > a.max_frames) {
            const int lo = s + a.min_frames + 1, hi = s + a.max_frames;  // the cut's window (s + min, s + max]; hi <= F - 1
            const int r0 = rid[lo], r1 = rid[hi];
            u64 best = 0;
            for (int r = r0 + tid; r <= r1; r += kVadThreads) {
                if (((m0 ^ r) & 1) == 0) {  // a silence run, clipped to the window: never empty
                    const int ca = bnd[r] > lo ? bnd[r] : lo, cb = bnd[r + 1] < hi + 1 ? bnd[r + 1] : hi + 1;
                    const u64 key = ((u64)(unsigned)(cb - ca) << 32) | (unsigned)r;  // longest, ties to the later run
                    best = key > best ? key : best;
                }
            }
            best = block_max_u64(best, sh_q);
            if (best) {
                const int r = (int)(unsigned)(best & 0xffffffffu);
                const int ca = bnd[r] > lo ? bnd[r] : lo, cb = bnd[r + 1] < hi + 1 ? bnd[r + 1] : hi + 1;
                c = (ca + cb) / 2;
            } else {  // no silence in the window: the first frame of least energy in its second half
                u64 least = 0;
                for (int t = s + a.max_frames / 2 + tid; t <= hi; t += kVadThreads) {
                    const u64 key = ~(((u64)vad_order_key(db[t]) << 32) | (unsigned)t);
                    least = key > least ? key : least;
                }
                least = ~block_max_u64(least, sh_q);
                c = (int)(unsigned)(least & 0xffffffffu);
            }
        }
        int st = s, en = c;
        bool keep = true;
        if (a.trim) {
            const int ra = rid[s], rb = rid[c - 1];
            const int first = ((m0 ^ ra) & 1) ? s : bnd[ra + 1];
            const int last = ((m0 ^ rb) & 1) ? c - 1 : bnd[rb] - 1;
            keep = first < c;
            st = first - a.pad > s ? first - a.pad : s;
            en = last + 1 + a.pad < c ? last + 1 + a.pad : c;
        }
        if (keep) {
            if (tid == 0 && n < a.max_segments) {
                seg_start[n] = st;
                seg_end[n] = en;
            }
            ++n;
        }
        s = c;
    }
    if (tid == 0) *count = n <= a.max_segments ? n : -n;
}

// One wave per (channel, segment): overlap[c][k] = the frames of [seg_start[c][k], seg_end[c][k]) in which the cleaned mask of any
// other channel is 1.  Runs behind vad_segments_kernel on the same stream; a count beyond max_segments covers the written ones.
__global__ __launch_bounds__(256) void vad_overlap_kernel(const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_end,
                                                          const int32_t* __restrict__ count, int C, int max_segments,
                                                          const unsigned char* __restrict__ ws, long slice, int32_t* __restrict__ overlap) {
    const int c = blockIdx.y, k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    int n = count[c];
    n = n < 0 || n > max_segments ? max_segments : n;
    if (k >= n) return;  // wave-uniform
    const int s = seg_start[(long)c * max_segments + k], e = seg_end[(long)c * max_segments + k];
    int acc = 0;
    for (int t = s + lane; t < e; t += 64) {
        int any = 0;
        for (int o = 0; o < C; ++o)
            if (o != c) any |= ws[(long)o * slice + t];
        acc += any;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) overlap[(long)c * max_segments + k] = acc;
}
}  // namespace

// A channel's part of the workspace: the mask (F bytes) at 0, F + 1 run boundaries at bnd_off, F run indices at rid_off, `bytes` in all
// -- what a one-channel launch touches at most; channel c's part starts at c * slice, so that every slice is 16-byte aligned.
struct VadLayout {
    long bnd_off, rid_off, bytes, slice;
};
static VadLayout vad_layout(long F) {
    const long bnd_off = (F + 15) & ~15L, rid_off = bnd_off + (((F + 1) * 4 + 15) & ~15L), bytes = rid_off + F * 4;
    return {bnd_off, rid_off, bytes, (bytes + 15) & ~15L};
}

size_t vad_workspace_bytes(long F) { return F < 1 || F > kVadMaxFrames ? 0 : (size_t)vad_layout(F).bytes; }

size_t vad_channels_workspace_bytes(int C, long F) {
    return C < 1 || C > kVadMaxChannels || F < 1 || F > kVadMaxFrames ? 0 : (size_t)C * (size_t)vad_layout(F).slice;
}

hipError_t launch_frame_energy_db(const float* wav, int C, long n, long stride, float* db, hipStream_t s) {
    if (n < kVadWindow || C < 1 || C > kVadMaxChannels || stride < n) return hipErrorInvalidValue;
    const long F = (n - (kVadWindow - kVadHop)) / kVadHop;  // 320 (F - 1) + 399 <= n - 1
    hipLaunchKernelGGL(frame_energy_db_kernel, dim3((unsigned)((F + 3) / 4), (unsigned)C), dim3(256), 0, s, wav, stride, F, db);
    return hipGetLastError();
}

hipError_t launch_vad_segments(const float* db, int C, const VadArgs& a, float crosstalk_db, int32_t* seg_start, int32_t* seg_end, int32_t* overlap,
                               int32_t* count, float* threshold_db, void* ws, hipStream_t s) {
    if (C < 1 || C > kVadMaxChannels || a.F < 1 || a.F > kVadMaxFrames || a.max_segments < 1 || a.min_frames < 1 || a.max_frames <= a.min_frames ||
        a.k_noise < 1 || a.k_peak < a.k_noise || a.k_peak > a.F || !(crosstalk_db >= 0.f))
        return hipErrorInvalidValue;
    const VadLayout l = vad_layout(a.F);
    const auto kernel = C == 1 ? vad_segments_kernel<true> : vad_segments_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)C), dim3(kVadThreads), 0, s, db, C, crosstalk_db, a, seg_start, seg_end, count, threshold_db,
                       static_cast<unsigned char*>(ws), l.slice, l.bnd_off, l.rid_off);
    if (const hipError_t e = hipGetLastError()) return e;
    if (overlap) {
        hipLaunchKernelGGL(vad_overlap_kernel, dim3((unsigned)((a.max_segments + 3) / 4), (unsigned)C), dim3(256), 0, s, seg_start, seg_end, count, C,
                           a.max_segments, static_cast<const unsigned char*>(ws), l.slice, overlap);
    }
    return hipGetLastError();
}

}  // namespace loco
