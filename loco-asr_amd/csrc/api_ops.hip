// C ABI (include/loco_asr.h), the operators that take no handle: single kernels behind loco_op_* for the parity tests and tools
// (LayerNorm, GEMMs, conv0, positional conv, attention, normalize, resample, split / permute), the GEMM knobs reload, and the
// long-form segmentation (VAD parameters and the two segment operators) and the error-rate operators (edit distance, n-best risk).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "loco_host.h"

using namespace loco;
using namespace loco::host;

extern "C" {

// ---- single operators ------------------------------------------------------------------------------------
int loco_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int32_t dim, float eps,
                      void* stream) {
    if (!x || !gamma || !beta || !y) return fail(LOCO_E_INVALID, "loco_op_layernorm: null argument");
    if (dim != 512 && dim != 768) return fail(LOCO_E_INVALID, "loco_op_layernorm: dim %d not in {512,768}", dim);
    HIP_TRY(launch_layernorm(x, gamma, beta, y, rows, dim, eps, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_gemm(const float* A, int64_t lda, const float* Wt, int64_t ldw, const float* bias, const float* R, int64_t ldr,
                 float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t nb1, int32_t nb2,
                 int64_t sA1, int64_t sA2, int64_t sC1, int64_t sC2, void* stream) {
    if (!A || !Wt || !C) return fail(LOCO_E_INVALID, "loco_op_gemm: null argument");
    if (K % 32 || (lda | ldw) & 3) return fail(LOCO_E_INVALID, "loco_op_gemm: K %% 32 and lda/ldw %% 4 must be 0");
    if (nb1 < 1 || nb2 < 1) return fail(LOCO_E_INVALID, "loco_op_gemm: batch counts must be >= 1");
    GemmArgs a{A, Wt, bias, R, C, M, N, K, lda, ldw, ldc, ldr, nb1, nb2, sA1, sA2, sC1, sC2, epilogue};
    HIP_TRY(launch_gemm(a, (hipStream_t)stream));
    return LOCO_OK;
}

size_t loco_conv0_scratch_bytes(int32_t B) { return conv0_scratch_bytes(B); }

int loco_op_conv0_gn_gelu(const float* wav, int32_t B, int64_t L, const float* w, const float* gn_w, const float* gn_b,
                          float* out, void* scratch, void* stream) {
    if (!wav || !w || !gn_w || !gn_b || !out || !scratch) return fail(LOCO_E_INVALID, "loco_op_conv0_gn_gelu: null argument");
    if (L < 10) return fail(LOCO_E_INVALID, "loco_op_conv0_gn_gelu: L < 10");
    HIP_TRY(launch_conv0_gn_gelu(wav, B, L, w, gn_w, gn_b, out, scratch, 1e-5f, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_conv0_gn_gelu_ex(const float* wav, int32_t B, int64_t L, const float* w, const float* gn_w, const float* gn_b, float* out,
                             void* out_hi, void* out_lo, float* range_slot, const int32_t* t0_clip, void* scratch, void* stream) {
    const char* fn = "loco_op_conv0_gn_gelu_ex";
    if (!wav || !w || !gn_w || !gn_b || !scratch) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if ((out_hi == nullptr) != (out_lo == nullptr)) return fail(LOCO_E_INVALID, "%s: out_hi and out_lo go together", fn);
    if ((out != nullptr) == (out_hi != nullptr)) return fail(LOCO_E_INVALID, "%s: exactly one of out and the plane pair", fn);
    if (L < 10) return fail(LOCO_E_INVALID, "%s: L < 10", fn);
    HIP_TRY(launch_conv0_gn_gelu(wav, B, L, w, gn_w, gn_b, out, scratch, 1e-5f, (hipStream_t)stream, out_hi, out_lo, range_slot, t0_clip));
    return LOCO_OK;
}

int loco_op_frame_counts(const int32_t* mask, int32_t B, int64_t L, int32_t* frames, void* stream) {
    if (!frames || B <= 0) return fail(LOCO_E_INVALID, "loco_op_frame_counts: invalid argument");
    HIP_TRY(launch_frame_counts(mask, B, L, frames, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_pos_conv(const float* h, const float* w_folded, const float* bias, const float* sin_table, const int32_t* frames,
                     float* out, int32_t B, int32_t T, void* stream) {
    if (!h || !w_folded || !bias || !sin_table || !out) return fail(LOCO_E_INVALID, "loco_op_pos_conv: null argument");
    HIP_TRY(launch_pos_conv(h, w_folded, bias, sin_table, frames, out, B, T, (hipStream_t)stream));
    return LOCO_OK;
}

size_t loco_normalize_scratch_bytes(int32_t B) { return B > 0 ? normalize_scratch_bytes(B) : 0; }

int loco_op_normalize_waveform(const float* wav, const int32_t* attention_mask, int32_t B, int64_t L, float padding_value, float* out,
                               void* scratch, size_t scratch_bytes, void* stream) {
    if (!wav || !out || !scratch || B <= 0 || L <= 0) return fail(LOCO_E_INVALID, "loco_op_normalize_waveform: null/invalid argument");
    if (scratch_bytes < normalize_scratch_bytes(B) || (reinterpret_cast<uintptr_t>(scratch) & 7))
        return fail(LOCO_E_WORKSPACE, "loco_op_normalize_waveform: scratch %zu < %zu bytes (or not 8-byte aligned)", scratch_bytes,
                    normalize_scratch_bytes(B));
    HIP_TRY(launch_normalize_waveform(wav, attention_mask, B, L, padding_value, out, scratch, (hipStream_t)stream));
    return LOCO_OK;
}

// ---- sample-rate conversion ("next" row f-4) -----------------------------------------------------------------------------
int loco_resample_design(int32_t sr_in, int32_t sr_out, int32_t* up, int32_t* down, int32_t* taps_per_phase, float* taps_host) {
    if (!up || !down || !taps_per_phase) return fail(LOCO_E_INVALID, "loco_resample_design: null argument");
    int L = 0, M = 0, K = 0;
    const int rc = resample_design(sr_in, sr_out, &L, &M, &K, taps_host);
    if (rc) return fail(LOCO_E_INVALID, "loco_resample_design: unsupported rates %d -> %d Hz", sr_in, sr_out);
    *up = L; *down = M; *taps_per_phase = K;
    return LOCO_OK;
}

int64_t loco_resample_length(int64_t n_in, int32_t up, int32_t down) {
    if (n_in <= 0 || up <= 0 || down <= 0) return 0;
    return (n_in * up + down - 1) / down;  // ceil(n * sr_out / sr_in): librosa.resample's n_samples (+ fix_length)
}

int loco_op_resample(const float* x, int32_t B, int64_t n_in, int64_t x_stride, const float* taps_dev, int32_t up, int32_t down,
                     int32_t taps_per_phase, float* y, int64_t n_out, int64_t y_stride, void* stream) {
    if (!x || !taps_dev || !y) return fail(LOCO_E_INVALID, "loco_op_resample: null argument");
    if (B <= 0 || n_in <= 0 || n_out <= 0 || n_out > loco_resample_length(n_in, up, down) || x_stride < n_in || y_stride < n_out ||
        (reinterpret_cast<uintptr_t>(taps_dev) & 15))
        return fail(LOCO_E_INVALID, "loco_op_resample: invalid shape (n_out must be <= ceil(n_in * up / down); taps 16-byte aligned)");
    HIP_TRY(launch_resample(x, B, n_in, x_stride, taps_dev, up, down, taps_per_phase, y, n_out, y_stride, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_split_f16(const float* x, void* hi, void* lo, int64_t n, void* stream) {
    if (!x || !hi || !lo || n <= 0 || (n & 3)) return fail(LOCO_E_INVALID, "loco_op_split_f16: invalid argument");
    HIP_TRY(launch_split_f16(x, hi, lo, n, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_gemm_f16x3(const void* Ahi, const void* Alo, int64_t lda, const void* Whi, const void* Wlo, int64_t ldw,
                       const float* bias, const float* R, int64_t ldr, float* C, void* Chi, void* Clo, int64_t ldc, int32_t M,
                       int32_t N, int32_t K, int32_t epilogue, int32_t nb1, int32_t nb2, int64_t sA1, int64_t sA2, int64_t sC1,
                       int64_t sC2, void* stream) {
    if (!Ahi || !Alo || !Whi || !Wlo || (!C && !Chi)) return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3: null argument");
    if (K % 32 || (lda | ldw) & 7) return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3: K %% 32 and lda/ldw %% 8 must be 0");
    if (Chi && ((ldc | sC1 | sC2) & 7))
        return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3: plane output needs ldc, sC1 and sC2 %% 8 == 0 (16-byte stores)");
    GemmSplitArgs a{(const _Float16*)Ahi, (const _Float16*)Alo, (const _Float16*)Whi, (const _Float16*)Wlo, bias, R, C,
                    (_Float16*)Chi, (_Float16*)Clo, M, N, K, lda, ldw, ldc, ldr, nb1, nb2, sA1, sA2, sC1, sC2, epilogue};
    HIP_TRY(launch_gemm_split(a, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_permute_conv_k(const float* w, float* out, int32_t N, int32_t taps, int32_t C, void* stream) {
    if (!w || !out) return fail(LOCO_E_INVALID, "loco_op_permute_conv_k: null argument");
    HIP_TRY(launch_permute_conv_k(w, out, N, taps, C, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_conv_gemm_f16x3(const void* Ahi, const void* Alo, int64_t lda, const void* Whi, const void* Wlo, float* C, void* Chi, void* Clo,
                            int32_t Tout, int32_t N, int32_t Cin, int32_t taps, int32_t epilogue, int32_t B, int64_t sA1, void* stream) {
    if (!Ahi || !Alo || !Whi || !Wlo || (!C && !Chi)) return fail(LOCO_E_INVALID, "loco_op_conv_gemm_f16x3: null argument");
    if (taps < 1 || taps > 3 || Cin % 64 || lda & 7) return fail(LOCO_E_INVALID, "loco_op_conv_gemm_f16x3: taps in 1..3, Cin %% 64 and lda %% 8");
    const int K = taps * Cin;
    GemmSplitArgs a{(const _Float16*)Ahi, (const _Float16*)Alo, (const _Float16*)Whi, (const _Float16*)Wlo, nullptr, nullptr, C,
                    (_Float16*)Chi, (_Float16*)Clo, Tout, N, K, lda, K, N, 0, B, 1, sA1, 0, (int64_t)Tout * N, 0, epilogue};
    a.ktaps = taps;
    HIP_TRY(launch_gemm_split(a, (hipStream_t)stream));
    return LOCO_OK;
}

size_t loco_gemm_splitk_bytes(void) { return kSplitKBytes; }

void loco_debug_reload_gemm_knobs(void) {
    reload_gemm_knobs();
    reload_attention_knobs();
}

int loco_op_gemm_f16x3_splitk(const void* Ahi, const void* Alo, int64_t lda, const void* Whi, const void* Wlo, int64_t ldw,
                              const float* bias, const float* R, int64_t ldr, float* C, void* Chi, void* Clo, int64_t ldc, int32_t M,
                              int32_t N, int32_t K, int32_t epilogue, void* splitk_ws, size_t splitk_bytes, void* stream) {
    if (!Ahi || !Alo || !Whi || !Wlo || (!C && !Chi) || !splitk_ws) return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3_splitk: null argument");
    if (K % 32 || (lda | ldw) & 7) return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3_splitk: K %% 32 and lda/ldw %% 8 must be 0");
    if (splitk_bytes < kSplitKBytes) return fail(LOCO_E_WORKSPACE, "loco_op_gemm_f16x3_splitk: workspace %zu < %zu bytes", splitk_bytes, kSplitKBytes);
    if (Chi && (ldc & 7)) return fail(LOCO_E_INVALID, "loco_op_gemm_f16x3_splitk: plane output needs ldc %% 8 == 0 (16-byte stores)");
    GemmSplitArgs a{(const _Float16*)Ahi, (const _Float16*)Alo, (const _Float16*)Whi, (const _Float16*)Wlo, bias, R, C,
                    (_Float16*)Chi, (_Float16*)Clo, M, N, K, lda, ldw, ldc, ldr, 1, 1, 0, 0, 0, 0, epilogue};
    a.splitk_ws = reinterpret_cast<float*>(splitk_ws);
    HIP_TRY(launch_gemm_split(a, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_gemm_f16x3_desc(const LocoGemmF16Desc* d, void* stream) {
    const char* fn = "loco_op_gemm_f16x3_desc";
    if (!d) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (d->struct_size != sizeof(LocoGemmF16Desc))
        return fail(LOCO_E_INVALID, "%s: struct_size = %u is not sizeof(LocoGemmF16Desc) = %zu", fn, d->struct_size, sizeof(LocoGemmF16Desc));
    if (!d->Ahi || !d->Alo || !d->Whi || !d->Wlo || (!d->C && !d->Chi)) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (d->K % 32 || (d->lda | d->ldw) & 7) return fail(LOCO_E_INVALID, "%s: K %% 32 and lda/ldw %% 8 must be 0", fn);
    if (d->epilogue < 0 || d->epilogue > 3) return fail(LOCO_E_INVALID, "%s: epilogue %d not in 0..3", fn, d->epilogue);
    if (d->terms != 2 && d->terms != 3) return fail(LOCO_E_INVALID, "%s: terms must be 2 or 3", fn);
    if ((d->Rhi == nullptr) != (d->Rlo == nullptr)) return fail(LOCO_E_INVALID, "%s: Rhi and Rlo go together", fn);
    if (d->Chi && ((d->ldc | d->sC1 | d->sC2 | d->qkv_stride) & 7))
        return fail(LOCO_E_INVALID, "%s: plane output needs ldc, sC1, sC2 and qkv_stride %% 8 == 0 (16-byte stores)", fn);
    if (d->splitk_ws && d->splitk_bytes < kSplitKBytes)
        return fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, d->splitk_bytes, kSplitKBytes);
    GemmSplitArgs a{(const _Float16*)d->Ahi, (const _Float16*)d->Alo, (const _Float16*)d->Whi, (const _Float16*)d->Wlo, d->bias, d->R, d->C,
                    (_Float16*)d->Chi, (_Float16*)d->Clo, d->M, d->N, d->K, d->lda, d->ldw, d->ldc, d->ldr, d->nb1, d->nb2, d->sA1, d->sA2,
                    d->sC1, d->sC2, d->epilogue};
    a.Rhi = (const _Float16*)d->Rhi;
    a.Rlo = (const _Float16*)d->Rlo;
    a.out_scale = d->out_scale;
    a.terms = d->terms;
    a.range_slot = d->range_slot;
    a.qkv_stride = d->qkv_stride;
    a.splitk_ws = reinterpret_cast<float*>(d->splitk_ws);
    a.co_scheduled = d->co_scheduled != 0;
    HIP_TRY(launch_gemm_split(a, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_pos_conv_f16x3(const float* h, const void* whi, const void* wlo, const float* bias, const float* sin_table, const int32_t* frames,
                           const int32_t* rows_clip, float out_scale, int32_t terms, void* ghi, void* glo, void* splitk_ws, size_t splitk_bytes,
                           float* out, int32_t B, int32_t T, void* stream) {
    const char* fn = "loco_op_pos_conv_f16x3";
    if (!h || !whi || !wlo || !bias || !sin_table || !ghi || !glo || !out) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (B <= 0 || T <= 0) return fail(LOCO_E_INVALID, "%s: B and T must be >= 1", fn);
    if (terms != 2 && terms != 3) return fail(LOCO_E_INVALID, "%s: terms must be 2 or 3", fn);
    if (splitk_ws && splitk_bytes < kSplitKBytes) return fail(LOCO_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, splitk_bytes, kSplitKBytes);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_group_major_split(h, ghi, glo, B, T, s, nullptr, rows_clip));
    // the launch of prenet_f16x3 (api_forward.hip)
    GemmSplitArgs a{};
    a.M = T; a.N = kPosCg; a.K = kPosK * kPosCg; a.epilogue = kEpiPosConv;
    a.Ahi = (const _Float16*)ghi; a.Alo = (const _Float16*)glo; a.Whi = (const _Float16*)whi; a.Wlo = (const _Float16*)wlo;
    a.bias = bias; a.R = h; a.C = out;
    a.lda = kPosCg; a.ldw = kPosK * kPosCg; a.ldc = kHidden; a.ldr = kHidden;
    a.nb1 = B; a.nb2 = kPosGroups;
    a.sA1 = (long)kPosGroups * (T + kPosK) * kPosCg; a.sA2 = (long)(T + kPosK) * kPosCg;
    a.sC1 = (long)T * kHidden; a.sC2 = kPosCg;
    a.sW2 = (long)kPosCg * kPosK * kPosCg; a.sBias2 = kPosCg;
    a.sin_table = sin_table; a.frames = frames; a.T = T;
    a.out_scale = out_scale; a.terms = terms;
    a.splitk_ws = reinterpret_cast<float*>(splitk_ws);
    HIP_TRY(launch_gemm_split(a, s));
    return LOCO_OK;
}

int loco_op_layernorm_f16x3(const float* x, const float* gamma, const float* beta, float* y, void* yhi, void* ylo, float* nonfinite_slot,
                            int64_t rows, int32_t dim, float eps, void* stream) {
    if (!x || !gamma || !beta || !yhi || !ylo) return fail(LOCO_E_INVALID, "loco_op_layernorm_f16x3: null argument");
    if (dim != 512 && dim != 768) return fail(LOCO_E_INVALID, "loco_op_layernorm_f16x3: dim %d not in {512,768}", dim);
    HIP_TRY(launch_layernorm(x, gamma, beta, y, rows, dim, eps, (hipStream_t)stream, yhi, ylo, nonfinite_slot));
    return LOCO_OK;
}

int loco_op_layernorm_f16x3_residual(const float* x, const void* rhi, const void* rlo, const float* gamma, const float* beta, float* y,
                                     void* yhi, void* ylo, float* nonfinite_slot, int64_t rows, int32_t dim, float eps, void* stream) {
    const char* fn = "loco_op_layernorm_f16x3_residual";
    if (!x || !rhi || !rlo || !gamma || !beta || !yhi || !ylo) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (dim != 512 && dim != 768) return fail(LOCO_E_INVALID, "%s: dim %d not in {512,768}", fn, dim);
    if ((reinterpret_cast<uintptr_t>(rhi) | reinterpret_cast<uintptr_t>(rlo)) & 7) return fail(LOCO_E_INVALID, "%s: rhi / rlo must be 8-byte aligned", fn);
    HIP_TRY(launch_layernorm(x, gamma, beta, y, rows, dim, eps, (hipStream_t)stream, yhi, ylo, nonfinite_slot, rhi, rlo));
    return LOCO_OK;
}

int loco_op_attention_f16x3(const void* qhi, const void* qlo, const void* khi, const void* klo, const void* vhi, const void* vlo,
                            const float* qp, const int32_t* frames, float* ctx, int32_t B, int32_t T, void* stream) {
    if (!qhi || !qlo || !khi || !klo || !vhi || !vlo || !qp || !ctx) return fail(LOCO_E_INVALID, "loco_op_attention_f16x3: null argument");
    HIP_TRY(launch_attention_f16x3((const _Float16*)qhi, (const _Float16*)qlo, (const _Float16*)khi, (const _Float16*)klo,
                                   (const _Float16*)vhi, (const _Float16*)vlo, qp, frames, nullptr, nullptr, ctx, B, T,
                                   (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_attention_f16x3_pe(const void* qhi, const void* qlo, const void* khi, const void* klo, const void* vhi, const void* vlo,
                               const void* pe_hi, const void* pe_lo, float pe_scale, float* qp_scratch, const int32_t* frames, float* ctx,
                               int32_t B, int32_t T, void* stream) {
    if (!qhi || !qlo || !khi || !klo || !vhi || !vlo || !pe_hi || !pe_lo || !qp_scratch || !ctx)
        return fail(LOCO_E_INVALID, "loco_op_attention_f16x3_pe: null argument");
    HIP_TRY(launch_attention_f16x3((const _Float16*)qhi, (const _Float16*)qlo, (const _Float16*)khi, (const _Float16*)klo,
                                   (const _Float16*)vhi, (const _Float16*)vlo, qp_scratch, frames, nullptr, nullptr, ctx, B, T,
                                   (hipStream_t)stream, (const _Float16*)pe_hi, (const _Float16*)pe_lo, pe_scale));
    return LOCO_OK;
}

int loco_op_attention_f16x3_planes(const void* qhi, const void* qlo, const void* khi, const void* klo, const void* vhi, const void* vlo,
                                   const void* pe_hi, const void* pe_lo, float pe_scale, float* qp, const int32_t* frames, void* ctx_hi,
                                   void* ctx_lo, int32_t B, int32_t T, void* stream) {
    if (!qhi || !qlo || !khi || !klo || !vhi || !vlo || !qp || !ctx_hi || !ctx_lo)
        return fail(LOCO_E_INVALID, "loco_op_attention_f16x3_planes: null argument");
    if ((pe_hi == nullptr) != (pe_lo == nullptr)) return fail(LOCO_E_INVALID, "loco_op_attention_f16x3_planes: pe_hi and pe_lo go together");
    HIP_TRY(launch_attention_f16x3((const _Float16*)qhi, (const _Float16*)qlo, (const _Float16*)khi, (const _Float16*)klo,
                                   (const _Float16*)vhi, (const _Float16*)vlo, qp, frames, (_Float16*)ctx_hi, (_Float16*)ctx_lo, nullptr, B, T,
                                   (hipStream_t)stream, (const _Float16*)pe_hi, (const _Float16*)pe_lo, pe_scale));
    return LOCO_OK;
}

int loco_op_attention_probs(const float* qkv, const float* qp, const int32_t* frames, float* probs, int32_t B, int32_t T, void* stream) {
    if (!qkv || !qp || !probs) return fail(LOCO_E_INVALID, "loco_op_attention_probs: null argument");
    HIP_TRY(launch_attention_probs(qkv, nullptr, nullptr, nullptr, nullptr, qp, frames, probs, B, T, 3, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_attention_probs_f16x3(const void* qhi, const void* qlo, const void* khi, const void* klo, const float* qp, const int32_t* frames,
                                  float* probs, int32_t B, int32_t T, int32_t terms, void* stream) {
    if (!qhi || !qlo || !khi || !klo || !qp || !probs) return fail(LOCO_E_INVALID, "loco_op_attention_probs_f16x3: null argument");
    if (terms != 2 && terms != 3) return fail(LOCO_E_INVALID, "loco_op_attention_probs_f16x3: terms must be 2 or 3");
    HIP_TRY(launch_attention_probs(nullptr, (const _Float16*)qhi, (const _Float16*)qlo, (const _Float16*)khi, (const _Float16*)klo, qp,
                                   frames, probs, B, T, terms, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_attention(const float* qkv, const float* qp, const int32_t* frames, float* ctx, int32_t B, int32_t T, void* stream) {
    if (!qkv || !qp || !ctx) return fail(LOCO_E_INVALID, "loco_op_attention: null argument");
    HIP_TRY(launch_attention(qkv, qp, frames, ctx, B, T, (hipStream_t)stream));
    return LOCO_OK;
}

// ---- long-form segmentation (segment.hip) ----
void loco_vad_default_params(LocoVadParams* p) {
    if (!p) return;
    *p = LocoVadParams{(uint32_t)sizeof(LocoVadParams), 1, 20.0, 1.0, 0.3, 0.1, 0.2, 0.10, 0.99, 10.0, -60.0, 15.0};
}

int loco_vad_frames(const LocoVadParams* p, int32_t* frames) {
    const char* fn = "loco_vad_frames";
    if (!p || !frames) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (p->struct_size != sizeof(LocoVadParams))
        return fail(LOCO_E_INVALID, "%s: struct_size = %u is not sizeof(LocoVadParams) = %zu", fn, p->struct_size, sizeof(LocoVadParams));
    const struct { const char* name; double v; } all[] = {
        {"max_segment_s", p->max_segment_s}, {"min_segment_s", p->min_segment_s}, {"min_silence_s", p->min_silence_s},
        {"min_speech_s", p->min_speech_s},   {"pad_s", p->pad_s},                 {"noise_quantile", p->noise_quantile},
        {"peak_quantile", p->peak_quantile}, {"margin_db", p->margin_db},         {"abs_floor_db", p->abs_floor_db},
        {"min_dynamic_db", p->min_dynamic_db}};
    for (const auto& f : all)
        if (!std::isfinite(f.v)) return fail(LOCO_E_INVALID, "%s: %s = %g is not finite", fn, f.name, f.v);
    if (p->max_segment_s > LOCO_VAD_MAX_SEGMENT_S)
        return fail(LOCO_E_INVALID, "%s: max_segment_s = %g exceeds %g s, what the decoder's 450 token positions hold at about 15 characters a second",
                    fn, p->max_segment_s, (double)LOCO_VAD_MAX_SEGMENT_S);
    for (int i = 1; i < 5; ++i)
        if (all[i].v < 0.0 || all[i].v > LOCO_VAD_MAX_SEGMENT_S)
            return fail(LOCO_E_INVALID, "%s: %s = %g is outside 0 .. %g s", fn, all[i].name, all[i].v, (double)LOCO_VAD_MAX_SEGMENT_S);
    const auto to_frames = [](double s) { return (int32_t)std::nearbyint(s * 50.0); };  // ties to even, as Python's round()
    const int32_t maxf = to_frames(p->max_segment_s), minf = to_frames(p->min_segment_s), sil = to_frames(p->min_silence_s);
    if (maxf < 2) return fail(LOCO_E_INVALID, "%s: max_segment_s = %g is below 2 frames (0.04 s)", fn, p->max_segment_s);
    if (minf < 1) return fail(LOCO_E_INVALID, "%s: min_segment_s = %g is below one frame (0.02 s)", fn, p->min_segment_s);
    if (minf >= maxf)
        return fail(LOCO_E_INVALID, "%s: min_segment_s = %g is not below max_segment_s = %g: the walk over cuts would make no progress", fn,
                    p->min_segment_s, p->max_segment_s);
    if (sil < 1) return fail(LOCO_E_INVALID, "%s: min_silence_s = %g is below one frame (0.02 s)", fn, p->min_silence_s);
    if (!(p->noise_quantile > 0.0 && p->noise_quantile < 1.0))
        return fail(LOCO_E_INVALID, "%s: noise_quantile = %g is outside (0, 1)", fn, p->noise_quantile);
    if (!(p->peak_quantile > 0.0 && p->peak_quantile < 1.0))
        return fail(LOCO_E_INVALID, "%s: peak_quantile = %g is outside (0, 1)", fn, p->peak_quantile);
    if (p->noise_quantile >= p->peak_quantile)
        return fail(LOCO_E_INVALID, "%s: noise_quantile = %g is not below peak_quantile = %g", fn, p->noise_quantile, p->peak_quantile);
    if (p->margin_db < 0.0) return fail(LOCO_E_INVALID, "%s: margin_db = %g is negative", fn, p->margin_db);
    if (p->min_dynamic_db < 0.0) return fail(LOCO_E_INVALID, "%s: min_dynamic_db = %g is negative", fn, p->min_dynamic_db);
    frames[0] = maxf;
    frames[1] = minf;
    frames[2] = sil;
    frames[3] = to_frames(p->min_speech_s);
    frames[4] = to_frames(p->pad_s);
    return LOCO_OK;
}

size_t loco_vad_workspace_bytes(int64_t F) { return vad_workspace_bytes((long)F); }
size_t loco_vad_channels_workspace_bytes(int32_t C, int64_t F) { return vad_channels_workspace_bytes((int)C, (long)F); }

// Both energy entries, fn = the entry's name; the mono entry is C = 1 with stride = n.
static int frame_energy_db_checked(const char* fn, const float* wav, int32_t C, int64_t n, int64_t stride, float* db, void* stream) {
    if (!wav || !db) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (C < 1 || C > kVadMaxChannels) return fail(LOCO_E_INVALID, "%s: C = %d is outside 1 .. %d channels", fn, C, kVadMaxChannels);
    if (n < kVadWindow) return fail(LOCO_E_INVALID, "%s: n = %lld samples is shorter than one frame (400)", fn, (long long)n);
    if (loco_output_frames(n) > kVadMaxFrames)
        return fail(LOCO_E_INVALID, "%s: n = %lld samples exceed %ld frames", fn, (long long)n, kVadMaxFrames);
    if (stride < n) return fail(LOCO_E_INVALID, "%s: stride = %lld is below n = %lld", fn, (long long)stride, (long long)n);
    HIP_TRY(launch_frame_energy_db(wav, (int)C, (long)n, (long)stride, db, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_frame_energy_db(const float* wav, int64_t n, float* db, void* stream) {
    return frame_energy_db_checked("loco_op_frame_energy_db", wav, 1, n, n, db, stream);
}

int loco_op_frame_energy_db_channels(const float* wav, int32_t C, int64_t n, int64_t stride, float* db, void* stream) {
    return frame_energy_db_checked("loco_op_frame_energy_db_channels", wav, C, n, stride, db, stream);
}

// Both segmentation entries, fn = the entry's name, need = the workspace the entry asks for; the mono entry is C = 1 with the gate off
// (+inf), no overlap and need = loco_vad_workspace_bytes(F), which is all a one-channel launch touches.
static int vad_segments_checked(const char* fn, const float* db, int32_t C, int64_t F, const LocoVadParams* params, float crosstalk_db,
                                int32_t* seg_start, int32_t* seg_end, int32_t* overlap, int32_t max_segments, int32_t* count, float* threshold_db,
                                void* workspace, size_t workspace_bytes, size_t need, void* stream) {
    if (!db || !params || !seg_start || !seg_end || !count || !threshold_db || !workspace) return fail(LOCO_E_INVALID, "%s: null argument", fn);
    if (C < 1 || C > kVadMaxChannels) return fail(LOCO_E_INVALID, "%s: C = %d is outside 1 .. %d channels", fn, C, kVadMaxChannels);
    if (!(crosstalk_db >= 0.f)) return fail(LOCO_E_INVALID, "%s: crosstalk_db = %g is NaN or negative (+inf switches the gate off)", fn, (double)crosstalk_db);
    if (F < 1 || F > kVadMaxFrames) return fail(LOCO_E_INVALID, "%s: F = %lld is outside 1 .. %ld frames", fn, (long long)F, kVadMaxFrames);
    if (max_segments < 1) return fail(LOCO_E_INVALID, "%s: max_segments = %d must be >= 1", fn, max_segments);
    int32_t fr[5];
    if (const int rc = loco_vad_frames(params, fr)) return rc;
    if (workspace_bytes < need) return fail(LOCO_E_INVALID, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    const auto rank = [F](double q) {
        const int64_t k = (int64_t)std::ceil(q * (double)F);
        return (int)(k < 1 ? 1 : (k > F ? F : k));
    };
    VadArgs a{(int)F, fr[0], fr[1], fr[2], fr[3], fr[4], params->trim ? 1 : 0, rank(params->noise_quantile), rank(params->peak_quantile),
              (float)params->margin_db, (float)params->abs_floor_db, (float)params->min_dynamic_db, max_segments};
    HIP_TRY(launch_vad_segments(db, (int)C, a, crosstalk_db, seg_start, seg_end, overlap, count, threshold_db, workspace, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_vad_segments(const float* db, int64_t F, const LocoVadParams* params, int32_t* seg_start, int32_t* seg_end, int32_t max_segments,
                         int32_t* count, float* threshold_db, void* workspace, size_t workspace_bytes, void* stream) {
    return vad_segments_checked("loco_op_vad_segments", db, 1, F, params, INFINITY, seg_start, seg_end, nullptr, max_segments, count, threshold_db,
                                workspace, workspace_bytes, vad_workspace_bytes((long)F), stream);
}

int loco_op_vad_segments_channels(const float* db, int32_t C, int64_t F, const LocoVadParams* params, float crosstalk_db, int32_t* seg_start,
                                  int32_t* seg_end, int32_t* overlap, int32_t max_segments, int32_t* count, float* threshold_db, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return vad_segments_checked("loco_op_vad_segments_channels", db, C, F, params, crosstalk_db, seg_start, seg_end, overlap, max_segments, count,
                                threshold_db, workspace, workspace_bytes, vad_channels_workspace_bytes((int)C, (long)F), stream);
}

// ---- error rates (edit_distance.hip) ----
static_assert(LOCO_EDIT_MAX_LEN == kEditMaxLen, "the header's cap is the kernel's");

int32_t loco_edit_max_len(void) { return kEditMaxLen; }

static bool misaligned(const void* p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }

int loco_op_edit_distance(const int32_t* symbols, int64_t n_symbols, const int32_t* spans, int32_t P, int32_t max_len, int32_t* counts,
                          void* stream) {
    const char* fn = "loco_op_edit_distance";
    if (!symbols) return fail(LOCO_E_INVALID, "%s: symbols is null", fn);
    if (!spans) return fail(LOCO_E_INVALID, "%s: spans is null", fn);
    if (!counts) return fail(LOCO_E_INVALID, "%s: counts is null", fn);
    if (P < 0) return fail(LOCO_E_INVALID, "%s: P = %d is negative", fn, P);
    if (n_symbols < 0 || n_symbols > INT32_MAX) return fail(LOCO_E_INVALID, "%s: n_symbols = %lld is outside 0 .. 2^31 - 1", fn, (long long)n_symbols);
    if (max_len < 0 || max_len > kEditMaxLen) return fail(LOCO_E_INVALID, "%s: max_len = %d is outside 0 .. %d", fn, max_len, kEditMaxLen);
    if (misaligned(symbols, 4)) return fail(LOCO_E_INVALID, "%s: symbols is not 4-byte aligned", fn);
    if (misaligned(spans, 16)) return fail(LOCO_E_INVALID, "%s: spans is not 16-byte aligned", fn);
    if (misaligned(counts, 4)) return fail(LOCO_E_INVALID, "%s: counts is not 4-byte aligned", fn);
    HIP_TRY(launch_edit_distance(symbols, (long)n_symbols, spans, P, max_len, counts, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_nbest_risk(const int32_t* counts, const int32_t* group_offsets, const double* weights, int32_t U, double* risk, int32_t* best,
                       void* stream) {
    const char* fn = "loco_op_nbest_risk";
    if (!counts) return fail(LOCO_E_INVALID, "%s: counts is null", fn);
    if (!group_offsets) return fail(LOCO_E_INVALID, "%s: group_offsets is null", fn);
    if (!risk) return fail(LOCO_E_INVALID, "%s: risk is null", fn);
    if (!best) return fail(LOCO_E_INVALID, "%s: best is null", fn);
    if (U < 0) return fail(LOCO_E_INVALID, "%s: U = %d is negative", fn, U);
    if (misaligned(counts, 4)) return fail(LOCO_E_INVALID, "%s: counts is not 4-byte aligned", fn);
    if (misaligned(group_offsets, 4)) return fail(LOCO_E_INVALID, "%s: group_offsets is not 4-byte aligned", fn);
    if (misaligned(best, 4)) return fail(LOCO_E_INVALID, "%s: best is not 4-byte aligned", fn);
    if (misaligned(weights, 8)) return fail(LOCO_E_INVALID, "%s: weights is not 8-byte aligned", fn);
    if (misaligned(risk, 8)) return fail(LOCO_E_INVALID, "%s: risk is not 8-byte aligned", fn);
    HIP_TRY(launch_nbest_risk(counts, group_offsets, weights, U, risk, best, (hipStream_t)stream));
    return LOCO_OK;
}

// ---- embedding neighbours (neighbors.hip) ----
static_assert(LOCO_TOPK_MAX_K == kTopkMaxK, "the header's cap is the kernel's");
static_assert(LOCO_TOPK_DOT == kTopkDot && LOCO_TOPK_COSINE == kTopkCosine && LOCO_TOPK_L2 == kTopkL2, "the header's metrics are the kernel's");

int32_t loco_topk_max_k(void) { return kTopkMaxK; }

size_t loco_topk_scratch_bytes(int64_t M, int64_t N, int32_t k) { return topk_scratch_bytes((long)M, (long)N, (int)k); }

int loco_op_row_norm2(const float* x, int64_t ldx, int64_t rows, int32_t dim, float* norm2, void* stream) {
    const char* fn = "loco_op_row_norm2";
    if (!x) return fail(LOCO_E_INVALID, "%s: x is null", fn);
    if (!norm2) return fail(LOCO_E_INVALID, "%s: norm2 is null", fn);
    if (dim != kHidden) return fail(LOCO_E_INVALID, "%s: dim = %d is not %d", fn, dim, kHidden);
    if (rows < 1 || rows > INT32_MAX) return fail(LOCO_E_INVALID, "%s: rows = %lld is outside 1 .. 2^31 - 1", fn, (long long)rows);
    if (ldx < kHidden) return fail(LOCO_E_INVALID, "%s: ldx = %lld is below %d", fn, (long long)ldx, kHidden);
    if (misaligned(x, 4) || misaligned(norm2, 4)) return fail(LOCO_E_INVALID, "%s: x / norm2 is not 4-byte aligned", fn);
    HIP_TRY(launch_row_norm2(x, (long)ldx, (long)rows, norm2, (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_topk(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* q_norm2, const float* k_norm2, const int32_t* exclude,
                 int64_t M, int64_t N, int32_t dim, int32_t k, int32_t metric, float* values, int32_t* indices, void* scratch,
                 size_t scratch_bytes, void* stream) {
    const char* fn = "loco_op_topk";
    if (!Q) return fail(LOCO_E_INVALID, "%s: Q is null", fn);
    if (!K) return fail(LOCO_E_INVALID, "%s: K is null", fn);
    if (!values) return fail(LOCO_E_INVALID, "%s: values is null", fn);
    if (!indices) return fail(LOCO_E_INVALID, "%s: indices is null", fn);
    if (!scratch) return fail(LOCO_E_INVALID, "%s: scratch is null", fn);
    if (dim != kHidden) return fail(LOCO_E_INVALID, "%s: dim = %d is not %d", fn, dim, kHidden);
    if (k < 1 || k > kTopkMaxK) return fail(LOCO_E_INVALID, "%s: k = %d is outside 1 .. %d", fn, k, kTopkMaxK);
    if (metric != kTopkDot && metric != kTopkCosine && metric != kTopkL2) return fail(LOCO_E_INVALID, "%s: metric = %d is not dot, cosine or l2", fn, metric);
    if (metric != kTopkDot && !q_norm2) return fail(LOCO_E_INVALID, "%s: q_norm2 is null (cosine and l2 need the squared norms)", fn);
    if (metric != kTopkDot && !k_norm2) return fail(LOCO_E_INVALID, "%s: k_norm2 is null (cosine and l2 need the squared norms)", fn);
    if (M < 1 || M > INT32_MAX) return fail(LOCO_E_INVALID, "%s: M = %lld is outside 1 .. 2^31 - 1", fn, (long long)M);
    if (N < 1 || N > INT32_MAX) return fail(LOCO_E_INVALID, "%s: N = %lld is outside 1 .. 2^31 - 1", fn, (long long)N);
    if ((M + 127) / 128 * topk_chunks((long)N) > INT32_MAX)
        return fail(LOCO_E_INVALID, "%s: M = %lld by N = %lld is more than 2^31 - 1 workgroups; split M", fn, (long long)M, (long long)N);
    if (ldq < kHidden || (ldq & 3) || ldq >= (1LL << 23)) return fail(LOCO_E_INVALID, "%s: ldq = %lld is not a multiple of 4 in 768 .. 2^23 - 1", fn, (long long)ldq);
    if (ldk < kHidden || (ldk & 3)) return fail(LOCO_E_INVALID, "%s: ldk = %lld is not a multiple of 4 of at least 768", fn, (long long)ldk);
    if (misaligned(Q, 16)) return fail(LOCO_E_INVALID, "%s: Q is not 16-byte aligned", fn);
    if (misaligned(K, 16)) return fail(LOCO_E_INVALID, "%s: K is not 16-byte aligned", fn);
    if (misaligned(scratch, 16)) return fail(LOCO_E_INVALID, "%s: scratch is not 16-byte aligned", fn);
    if (misaligned(values, 4) || misaligned(indices, 4) || misaligned(q_norm2, 4) || misaligned(k_norm2, 4) || misaligned(exclude, 4))
        return fail(LOCO_E_INVALID, "%s: values / indices / q_norm2 / k_norm2 / exclude is not 4-byte aligned", fn);
    const size_t need = topk_scratch_bytes((long)M, (long)N, (int)k);
    if (scratch_bytes < need) return fail(LOCO_E_WORKSPACE, "%s: scratch %zu < %zu bytes", fn, scratch_bytes, need);
    HIP_TRY(launch_topk(Q, (long)ldq, K, (long)ldk, q_norm2, k_norm2, exclude, (long)M, (long)N, (int)k, (int)metric, values, indices, scratch,
                        (hipStream_t)stream));
    return LOCO_OK;
}

int loco_op_group_mean(const float* rows, int64_t ld, int64_t n_rows, const int32_t* index, const int64_t* offsets, int64_t G, int32_t dim,
                       float* out, int64_t ldo, int32_t* count, void* stream) {
    const char* fn = "loco_op_group_mean";
    if (!rows) return fail(LOCO_E_INVALID, "%s: rows is null", fn);
    if (!offsets) return fail(LOCO_E_INVALID, "%s: offsets is null", fn);
    if (!out) return fail(LOCO_E_INVALID, "%s: out is null", fn);
    if (dim != kHidden) return fail(LOCO_E_INVALID, "%s: dim = %d is not %d", fn, dim, kHidden);
    if (G < 1 || G > INT32_MAX) return fail(LOCO_E_INVALID, "%s: G = %lld is outside 1 .. 2^31 - 1", fn, (long long)G);
    if (n_rows < 1) return fail(LOCO_E_INVALID, "%s: n_rows = %lld is below 1", fn, (long long)n_rows);
    if (ld < kHidden || (ld & 3)) return fail(LOCO_E_INVALID, "%s: ld = %lld is not a multiple of 4 of at least 768", fn, (long long)ld);
    if (ldo < kHidden || (ldo & 3)) return fail(LOCO_E_INVALID, "%s: ldo = %lld is not a multiple of 4 of at least 768", fn, (long long)ldo);
    if (misaligned(rows, 16)) return fail(LOCO_E_INVALID, "%s: rows is not 16-byte aligned", fn);
    if (misaligned(out, 16)) return fail(LOCO_E_INVALID, "%s: out is not 16-byte aligned", fn);
    if (misaligned(offsets, 8)) return fail(LOCO_E_INVALID, "%s: offsets is not 8-byte aligned", fn);
    if (misaligned(index, 4) || misaligned(count, 4)) return fail(LOCO_E_INVALID, "%s: index / count is not 4-byte aligned", fn);
    HIP_TRY(launch_group_mean(rows, (long)ld, (long)n_rows, index, offsets, (long)G, out, (long)ldo, count, (hipStream_t)stream));
    return LOCO_OK;
}

}  // extern "C"
