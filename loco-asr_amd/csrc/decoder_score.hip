// Scores of the text decoder (include/loco_asr.h, loco_decoder_score): from logits to per-token log-probabilities, per-sequence sums
// and the mean cross-entropy HF's labels= path returns.
//   token_logprob_kernel  one wave per row of logits: log_softmax(row)[target], the target given or the row's argmax
//   score_reduce_kernel   per sequence the sum and the count of its valid positions; loss = -(sum of sums) / (sum of counts)
// A row's log-probability is a pure function of its V numbers, bit for bit: the lanes walk the row lane-strided in a fixed order and
// meet in xor butterflies (loco_kernels.h; the argmax's, by the decode step's rule, in decoder_common.h) whose two operands every lane
// pair adds (or compares) symmetrically, so all 64 lanes hold the same value and nothing depends on the row's place, on M or on the
// other rows.  The reduction's order depends on (B, S) only.  No atomics; neither kernel allocates, synchronises or depends on the host.
#include <climits>

#include "decoder_common.h"

namespace loco {

namespace {

// 256 threads = 4 waves = 4 rows.  Lane l reads columns l, l + 64, ... < V and never another.  -inf entries add exp(-inf) = 0; a row
// whose maximum is +inf or -inf gives inf - inf = NaN and a NaN entry a NaN sum, as torch.log_softmax does.
__global__ __launch_bounds__(256) void token_logprob_kernel(const float* __restrict__ logits, long ld, const int32_t* __restrict__ targets, long M,
                                                            int V, int ignore_index, float* __restrict__ logprob, int32_t* __restrict__ chosen) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* x = logits + row * ld;
    int target = 0;
    if (targets) {
        target = targets[row];
        if (target == ignore_index) {
            if (lane == 0) {
                logprob[row] = 0.f;
                if (chosen) chosen[row] = target;
            }
            return;
        }
    }
    float mx = -INFINITY, bv = -INFINITY;
    int bi = INT_MAX;  // a lane without a column: loses to every real entry, an all -inf row's index 0 included
    for (int n = lane; n < V; n += 64) {
        const float v = x[n];
        mx = fmaxf(mx, v);
        if (argmax_better(v, n, bv, bi)) bv = v, bi = n;
    }
    mx = wave_max(mx);
    wave_argmax(bv, bi);
    const float sum = row_exp_sum(x, V, lane, mx);
    if (!targets) target = bi;
    // a label outside [0, V) is never an index: the row is NaN and counts, so the loss says so
    const float xt = (target >= 0 && target < V) ? x[target] : NAN;
    if (lane == 0) {
        logprob[row] = row_logprob(xt, mx, sum);
        if (chosen) chosen[row] = target;
    }
}

// One workgroup of 16 waves, a wave per sequence (b, b + 16, ...): lane l adds positions l, l + 64, ... of the sequence in double, the
// lanes meet in a butterfly; a wave adds its sequences in order of b, thread 0 the 16 waves in order.
__global__ __launch_bounds__(1024) void score_reduce_kernel(const float* __restrict__ logprob, const int32_t* __restrict__ targets, int B, int S,
                                                            int ignore_index, float* __restrict__ seq_logprob, int32_t* __restrict__ seq_count,
                                                            float* __restrict__ loss) {
    __shared__ double sum_s[16];
    __shared__ long cnt_s[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double wsum = 0.0;
    long wcnt = 0;
    for (int b = wave; b < B; b += 16) {
        double s = 0.0;
        int c = 0;
        for (int t = lane; t < S; t += 64) {
            const long i = (long)b * S + t;
            const bool valid = !targets || targets[i] != ignore_index;
            if (valid) s += (double)logprob[i], c += 1;
        }
        s = wave_sum(s);
        c = wave_sum(c);
        if (lane == 0) {
            if (seq_logprob) seq_logprob[b] = (float)s;
            if (seq_count) seq_count[b] = c;
        }
        wsum += s;
        wcnt += c;
    }
    if (lane == 0) sum_s[wave] = wsum, cnt_s[wave] = wcnt;
    __syncthreads();
    if (threadIdx.x == 0 && loss) {
        double total = 0.0;
        long n = 0;
        for (int w = 0; w < 16; ++w) total += sum_s[w], n += cnt_s[w];
        loss[0] = (float)(-total / (double)n);  // no valid token: -0 / 0 = NaN, as torch's mean over none
    }
}

}  // namespace

hipError_t launch_token_logprob(const float* logits, long ld, const int32_t* targets, long M, int V, int ignore_index, float* logprob,
                                int32_t* chosen, hipStream_t s) {
    if (!logits || !logprob || M < 1 || M > INT_MAX || V < 1 || ld < V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(token_logprob_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, logits, ld, targets, M, V, ignore_index, logprob, chosen);
    return hipGetLastError();
}

hipError_t launch_score_reduce(const float* logprob, const int32_t* targets, int B, int S, int ignore_index, float* seq_logprob,
                               int32_t* seq_count, float* loss, hipStream_t s) {
    if (!logprob || B < 1 || S < 1 || (long)B * S > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_reduce_kernel, dim3(1), dim3(1024), 0, s, logprob, targets, B, S, ignore_index, seq_logprob, seq_count, loss);
    return hipGetLastError();
}

}  // namespace loco
