// Slot state of the decoder pool (include/loco_asr.h, loco_decoder_pool_*): every slot decodes one utterance at its own position, and a
// slot whose utterance has ended is handed to the next one.  The kernels here keep that state; the step's products run on the
// weight-streaming GEMM and the attention kernel of decoder.hip.
//   pool_init_kernel    every slot free
//   pool_admit_kernel   slot := <s>, position 0, its cap and frame count, open
//   pool_embed_kernel   token pos[r] of every open slot + sinusoid position; derives the step's key counts and cache rows; zeros for
//                       slots that are not open
//   pool_select_kernel  argmax of the open slots, append, finish on </s> or at the cap, advance
// A slot that is not open reads and writes nothing of its own in a step: its row is zeros in, key counts 0, no cache row, no token.
// No kernel allocates, synchronises or depends on the host.  A token's position and the argmax are decoder_common.h's rules, as in generate.
#include "decoder_common.h"

namespace loco {

namespace {

__global__ __launch_bounds__(64) void pool_init_kernel(PoolState p) {
    const int r = threadIdx.x;
    if (r < p.slots) {
        p.status[r] = kPoolFree;
        p.pos[r] = 0;
        p.cap[r] = 2;
        p.frames[r] = 0;
        p.lengths[r] = 0;
        p.self_count[r] = 0;
        p.cross_count[r] = 0;
        p.kv_row[r] = -1;
        p.cur[r] = kDecPadToken;
        p.cnt[r] = 0;
    }
    if (r < 4) p.poll[r] = 0;
}

__global__ __launch_bounds__(64) void pool_admit_kernel(PoolState p, PoolAdmit a, const int32_t* __restrict__ frames, int start) {
    const int i = threadIdx.x;
    if (i < a.n) {
        const int r = a.slot[i];
        p.tokens[(long)r * p.S_max] = start;
        p.cur[r] = start;
        p.cnt[r] = start != kDecPadToken;
        p.pos[r] = 0;
        p.cap[r] = a.cap[i];
        p.frames[r] = min(max(frames ? frames[i] : a.rows[i], 0), a.rows[i]);  // never beyond the rows that were projected
        p.lengths[r] = 1;
        p.status[r] = kPoolOpen;
    }
    __syncthreads();
    const unsigned long long open = __ballot(i < p.slots && p.status[i] == kPoolOpen);
    if (i == 0) p.poll[0] = __popcll(open);
}

// cur[r] is the token slot r consumes (token pos[r] of its buffer) and cnt[r] the non-pad tokens of its utterance up to and including
// it: the select kernel keeps both, so this kernel's loads of the slot's state are independent of one another and only the embedding
// rows wait for them (the chain dec_embed_step_kernel has).
__global__ __launch_bounds__(256) void pool_embed_kernel(PoolState p, const float* __restrict__ embed, int vocab, const float* __restrict__ table,
                                                         int table_rows, float* __restrict__ x, int max_pos, int max_frames) {
    const int r = blockIdx.x;
    const int t = p.pos[r], status = p.status[r], raw = p.cur[r], cnt = p.cnt[r], frames = p.frames[r];
    // a slot takes part in a step iff it is open AND its position leaves room for the token the step writes (pos + 1 < S_max): state
    // that loco_decoder_pool_init never wrote cannot send a store outside the buffers
    const bool live = status == kPoolOpen && t >= 0 && t + 1 < p.S_max && t <= max_pos;
    float* dst = x + (long)r * kHidden;
    if (!live) {
        if (threadIdx.x == 0) {
            p.self_count[r] = 0;
            p.cross_count[r] = 0;
            p.kv_row[r] = -1;
        }
        for (int c = threadIdx.x; c < kHidden; c += 256) dst[c] = 0.f;
        return;
    }
    if (threadIdx.x == 0) {
        p.self_count[r] = t + 1;
        p.cross_count[r] = min(frames, max_frames);
        p.kv_row[r] = t;
    }
    dec_embed_row(raw, raw != kDecPadToken, cnt, embed, vocab, table, table_rows, dst);
}

// One workgroup of 16 waves, a wave per slot (slots r, r + 16, ...): the lanes share the row's logits and meet in a butterfly, so the
// row is read coalesced.  kv_row[r] >= 0 marks the slots the step's embed kernel took as live.
__global__ __launch_bounds__(1024) void pool_select_kernel(PoolState p, const float* __restrict__ logits, int vocab, int eos) {
    __shared__ int open_s[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int open = 0;
    for (int r = wave; r < p.slots; r += 16) {
        const int t = p.kv_row[r], cap = p.cap[r], cnt = p.cnt[r], status = p.status[r];
        const float* l = logits + (long)r * vocab;
        int bi = min(lane, vocab - 1);
        float bv = l[bi];
        for (int n = lane + 64; n < vocab; n += 64) {
            const float v = l[n];
            if (argmax_better(v, n, bv, bi)) bv = v, bi = n;
        }
        wave_argmax(bv, bi);
        if (t >= 0) {
            const bool done = bi == eos || t + 2 >= cap || t + 2 >= p.S_max;
            if (lane == 0) {
                p.tokens[(long)r * p.S_max + t + 1] = bi;
                p.lengths[r] = t + 2;
                if (done) {
                    p.status[r] = kPoolFinished;
                } else {
                    p.pos[r] = t + 1;
                    p.cur[r] = bi;
                    p.cnt[r] = cnt + (bi != kDecPadToken);
                }
            }
            open += !done;
        } else if (status == kPoolOpen) {
            open += 1;  // open but outside this step's bounds: the caller's bound was too small; the slot waits
        }
    }
    if (lane == 0) open_s[wave] = open;
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < 16; ++w) n += open_s[w];
        p.poll[0] = n;
    }
}

}  // namespace

hipError_t launch_pool_init(const PoolState& p, hipStream_t s) {
    if (p.slots <= 0 || p.slots > kSkinnyMaxM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_init_kernel, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_pool_admit(const PoolState& p, const PoolAdmit& a, const int32_t* frames, int start, hipStream_t s) {
    if (p.slots <= 0 || p.slots > kSkinnyMaxM || a.n <= 0 || a.n > p.slots) return hipErrorInvalidValue;
    for (int i = 0; i < a.n; ++i)
        if (a.slot[i] < 0 || a.slot[i] >= p.slots || a.cap[i] < 2 || a.cap[i] > p.S_max || a.rows[i] < 1 || a.rows[i] > p.T_cap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_admit_kernel, dim3(1), dim3(64), 0, s, p, a, frames, start);
    return hipGetLastError();
}

hipError_t launch_pool_embed(const PoolState& p, const float* embed, int vocab, const float* table, int table_rows, float* x, int max_pos,
                             int max_frames, hipStream_t s) {
    if (p.slots <= 0 || p.slots > kSkinnyMaxM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_embed_kernel, dim3(p.slots), dim3(256), 0, s, p, embed, vocab, table, table_rows, x, max_pos, max_frames);
    return hipGetLastError();
}

hipError_t launch_pool_select(const PoolState& p, const float* logits, int vocab, int eos, hipStream_t s) {
    if (p.slots <= 0 || p.slots > kSkinnyMaxM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_select_kernel, dim3(1), dim3(1024), 0, s, p, logits, vocab, eos);
    return hipGetLastError();
}

}  // namespace loco
