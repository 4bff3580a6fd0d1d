/*
 * loco_asr.h -- C ABI of the MI355X-native SpeechT5 speech-encoder embedding path.
 *
 * What this boundary replaces.  The reference has no FFI of its own: its seam is a Python
 * attribute path on a HuggingFace module,
 *
 *     out = model.speecht5.encoder(**audios)                      (extract_speecht5_base_embeddings_slurp.py:108,
 *     embeddings = out.last_hidden_state                           extract_speecht5_finetuned_embeddings_slurp.py:104-106)
 *     model.speecht5.encoder.wrapped_encoder.load_state_dict(...)  (extract_speecht5_base_embeddings_slurp.py:99)
 *     model.speecht5.encoder.prenet.load_state_dict(...)           (extract_speecht5_base_embeddings_slurp.py:100)
 *
 * i.e. transformers' SpeechT5EncoderWithSpeechPrenet.forward (modeling_speecht5.py:1339-1358).  The
 * entry points below are what a binding for that seam needs: create / load weights by their
 * HuggingFace state-dict key / query workspace / forward on raw device pointers / destroy.  The
 * Python host side (loco-asr_amd/encoder.py) binds them with ctypes and re-exposes the HF module
 * contract; INTEGRATION.md shows the stub.
 *
 * Conventions: plain C types only; every buffer is caller-owned DEVICE memory (gfx950) unless a
 * parameter says "host"; nothing here allocates, synchronises the host or spawns threads inside
 * loco_forward; all work is enqueued on the hipStream_t passed in (void* so that this header needs no
 * HIP include).  Functions returning int give 0 on success and a negative LOCO_E_* code otherwise;
 * loco_last_error() returns the message of the calling thread's last failure.
 */
#ifndef LOCO_ASR_H
#define LOCO_ASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOCO_ABI_VERSION 1

enum {
    LOCO_OK = 0,
    LOCO_E_INVALID = -1,   /* bad argument (shape, null pointer, unknown key) -- HF raises ValueError here */
    LOCO_E_STATE = -2,     /* weights missing / not finalized */
    LOCO_E_WORKSPACE = -3, /* workspace too small */
    LOCO_E_HIP = -4,       /* a HIP runtime call failed */
    LOCO_E_RANGE = -5      /* an activation left the range precision mode f16x3 represents (loco_forward_status) */
};

/* Model hyper-parameters = transformers SpeechT5Config defaults (configuration_speecht5.py:142-199),
 * the configuration of "microsoft/speecht5_asr" that both reference scripts load.  Only `layers` may
 * be lowered (tests); the kernels are specialised for the other values and loco_create rejects
 * anything else. */
typedef struct loco_config {
    int32_t struct_size; /* sizeof(loco_config), for ABI checks */
    int32_t hidden;      /* 768 */
    int32_t heads;       /* 12  (head_dim 64) */
    int32_t ffn;         /* 3072 */
    int32_t layers;      /* 12 */
    int32_t conv_dim;    /* 512; conv kernels (10,3,3,3,3,2,2), strides (5,2,2,2,2,2,2) */
    int32_t pos_conv_kernel; /* 128 */
    int32_t pos_conv_groups; /* 16 */
    int32_t rel_max;     /* 160: relative positions clipped to [-160, 159] */
    float ln_eps;        /* 1e-5 */
} loco_config;

typedef struct loco_encoder loco_encoder; /* opaque */

int loco_abi_version(void);
const char* loco_last_error(void);
void loco_default_config(loco_config* cfg);

/* Lifetime.  loco_create binds the handle to the current HIP device. */
loco_encoder* loco_create(const loco_config* cfg);
void loco_destroy(loco_encoder* enc);

/* Weight loading -- the C side of the two load_state_dict calls.  `key` is the HuggingFace name
 * including its sub-module prefix ("prenet.feature_encoder.conv_layers.0.conv.weight",
 * "wrapped_encoder.layers.3.attention.q_proj.bias", ...).  Both spellings of the weight-normed
 * positional conv are accepted (transformers 4.30.2 "...conv.weight_g/_v"; 5.x
 * "...conv.parametrizations.weight.original0/1").  "prenet.masked_spec_embed" and
 * "prenet.pos_sinusoidal_embed.weights" (carried by the reference's pickled dicts,
 * map_speecht5_hf.py:164-166) are accepted; the former is unused in eval, the latter replaces the
 * internally generated table when its row count suffices.  `data` is fp32, device or host memory
 * (copied with hipMemcpyDefault); the library keeps its own re-laid-out copy, so the caller may free
 * `data` on return.  Returns LOCO_E_INVALID for an unknown key or a shape mismatch. */
int loco_set_weight(loco_encoder* enc, const char* key, const float* data, const int64_t* shape, int ndim);

/* Number of tensors still missing (0 = complete); when `buf` is non-null their names are written to it,
 * comma separated, truncated to `buflen`. */
int loco_missing_weights(const loco_encoder* enc, char* buf, size_t buflen);

/* Fold weight-norm, fuse q/k/v (+ the 1/8 query scaling), re-lay conv weights tap-major.  Must be
 * called after the last loco_set_weight and before loco_forward; idempotent. */
int loco_finalize_weights(loco_encoder* enc, void* stream);

/* floor((n-k)/s)+1 chained over the seven conv layers (modeling_speecht5.py:585-598); <= 0 when the
 * clip is shorter than one frame (400 samples). */
int64_t loco_output_frames(int64_t n_samples);

/* Bytes of scratch loco_forward needs for a [B, L] batch (256-byte aligned carve-outs included; the first 3 KiB hold the
 * forward's device-side range words). */
size_t loco_workspace_bytes(const loco_encoder* enc, int32_t B, int64_t L);

/* Forward = SpeechT5EncoderWithSpeechPrenet.forward in eval mode.
 *   wav            f32 [B, L]   zero-padded waveforms (device)
 *   attention_mask i32 [B, L]   1 = sample present, 0 = padding (device), or NULL = all present
 *   out            f32 [B, T, 768], T = loco_output_frames(L): last_hidden_state, padded frames included
 *                  exactly as HF computes them (the reference pickles them, ...base...py:109-113)
 *   out_frames     i32 [B] valid frame count per clip (device), may be NULL
 *   hidden_states  NULL, or host array of layers+1 device pointers f32 [B,T,768] receiving the input of
 *                  every layer and the final output (HF output_hidden_states=True, modeling:1287-1313)
 *   workspace      >= loco_workspace_bytes(enc, B, L) bytes (device)
 * Asynchronous: everything is enqueued on `stream` (and, for large batches, on a second stream joined back to it, see
 * loco_set_streams); nothing is allocated and the host is never blocked.
 * Concurrency contract of THIS entry point: its numeric-range status (below) lives in the handle, so forwards enqueued
 * through loco_forward / loco_forward_checked / loco_forward_text must not overlap -- not on two host threads, and not on two
 * streams without a dependency -- and loco_forward_status describes the MOST RECENT of them only (enqueue two back to back
 * on one stream and the first one's status is gone).  For several forwards of one handle in flight together use
 * loco_forward_async, which keeps everything a forward mutates in the caller's workspace and status block.
 */
int loco_forward(loco_encoder* enc, const float* wav, const int32_t* attention_mask, int32_t B, int64_t L,
                 float* out, int32_t* out_frames, float* const* hidden_states, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- numeric range of precision mode f16x3 (the default, loco_set_precision) -----------------------------------------------
 * In that mode every GEMM operand is carried as two fp16 planes, hi = fp16(x) and lo = fp16(x - hi): 22 significant bits
 * while lo is a normal fp16 number, an ABSOLUTE error floor of 2^-25 below that, and hi = inf from |x| >= 65520 on.
 *   Weights are immune: at loco_finalize_weights each tensor is stored as W * 2^k, k chosen so that max|W| lands in
 *     [2^13, 2^14), and the GEMM undoes the power of two exactly -- checkpoints with weights of 1e-7 or of 1e+4 load alike.
 *   Activations are guaranteed to fp32 class (<= 2e-5 relative L2 of an fp64 evaluation, tests/test_gpu_range.py) as long as
 *     the LARGEST element of every tensor that is stored as planes -- conv-stack outputs, LayerNorm outputs, q|k|v, the
 *     attention context, the GELU'd feed-forward intermediate -- lies in [2^-6, 65504).  Every producing kernel folds
 *     max|x| of what it writes (taken on the fp32 value, before conversion) into a status word of its stage; the words
 *     follow the forward to host memory on its stream.
 * loco_forward itself is asynchronous and therefore cannot know; after the stream has completed it,
 *   loco_forward_status   returns LOCO_OK, or LOCO_E_RANGE with a message naming the first stage outside the range and its
 *                         max|x| (also copied to `buf` when given).  In that case the output may hold inf / NaN (overflow) or
 *                         be less accurate than fp32 class (underflow) and must not be used.
 *   loco_forward_range    reads one stage's max|x| (diagnostics); returns the number of stages of the last forward.
 *   loco_forward_checked  = loco_forward + hipStreamSynchronize + loco_forward_status, and, under the default policy 1, a
 *                         second pass of the same batch on the exact-fp32 MFMA kernels of this library (precision mode 0,
 *                         ~2.5x slower, no range limit beyond fp32's own) when the first left the range; *used_fp32 tells.
 *                         With loco_set_range_policy(enc, 0) it returns LOCO_E_RANGE instead.  This is the entry point
 *                         the Python module calls: a caller never sees NaNs caused by the fp16 planes.
 * Inputs that contain inf / NaN themselves propagate as in HF (they are not a range error of this library). */
int loco_forward_status(loco_encoder* enc, char* buf, size_t buflen);
int loco_forward_range(const loco_encoder* enc, int32_t stage, float* amax, int32_t* layer, char* name, size_t namelen);
int loco_set_range_policy(loco_encoder* enc, int policy);
int loco_forward_checked(loco_encoder* enc, const float* wav, const int32_t* attention_mask, int32_t B, int64_t L,
                         float* out, int32_t* out_frames, float* const* hidden_states, void* workspace,
                         size_t workspace_bytes, void* stream, int32_t* used_fp32);

/* ---- several forwards of one handle in flight: a status block per forward ---------------------------------------------------
 * The reference encodes one batch of two utterances at a time (batch_size = 2, shuffle=False,
 * /root/reference/speech_text/extract_speecht5_base_embeddings_slurp.py:67-68); a pair of 5 s clips is ~125 kernel launches of
 * 5-16 us each and cannot fill 256 CUs.  Batch composition is part of the function (GroupNorm over the padded axis), so the
 * pairs must stay what they are -- but nothing orders pair k+1 behind pair k.  loco_forward_async is loco_forward with every
 * piece of per-forward state moved out of the handle:
 *   - the device range words sit in the first bytes of `workspace` (loco_workspace_bytes includes them),
 *   - the host side of the status -- stage names, arithmetic mode, and the target of the device-to-host copy that follows the
 *     forward on `stream` -- is the caller's `status` block: loco_status_bytes() bytes of HOST memory, 8-byte aligned, pinned
 *     (hipHostMalloc / torch pin_memory) if the copy is to be asynchronous, untouched by the caller until `stream` has
 *     completed the forward,
 *   - `precision` is an argument (-1 = the handle's current loco_set_precision mode), so a range fallback re-runs ONE batch on
 *     the exact-fp32 kernels without switching the handle under the other forwards in flight.
 * Forwards with different (workspace, status, out) triples may be enqueued on different streams and from different host threads
 * at the same time; the handle is only read.  (Exceptions, all one-time or diagnostic: a clip longer than any before grows the
 * sinusoid table -- under a lock, blocking that one call until the new table is complete, the old table staying alive for the
 * forwards already enqueued; profiling, taps and hidden_states remain single-caller features; the second stream of
 * loco_set_streams is shared, its use is serialised.)
 *   loco_status_check   after `stream` has completed the forward: LOCO_OK, or LOCO_E_RANGE with the message naming the first
 *                       stage outside the range (the output must then not be used: re-run the batch with precision 0);
 *                       LOCO_E_INVALID when `status` was not filled by a successful loco_forward_async.
 *   loco_status_range   one stage's max|x| (diagnostics), as loco_forward_range. */
size_t loco_status_bytes(void);
int loco_forward_async(loco_encoder* enc, int precision, const float* wav, const int32_t* attention_mask, int32_t B, int64_t L,
                       float* out, int32_t* out_frames, float* const* hidden_states, void* workspace, size_t workspace_bytes,
                       void* stream, void* status);
int loco_status_check(const void* status, char* buf, size_t buflen);

/* ---- packed forward: G reference batches in ONE launch sequence ---------------------------------------------------------------
 * The reference's loop encodes batch after batch of two utterances (batch_size = 2, shuffle=False,
 * /root/reference/speech_text/extract_speecht5_base_embeddings_slurp.py:51-68 collate_fn + DataLoader, :108 the forward).  A pair
 * of 2-6 s clips is a few hundred frames; every GEMM of it is a handful of tiles.  Batch composition is part of the function --
 * GroupNorm statistics run over the padded time axis of the batch (HF modeling_speecht5.py:275-279), the positional conv sees
 * zeros where the batch ends (:389-397) -- so the batches cannot simply be merged.  What CAN be merged is the launch sequence:
 * loco_forward_packed runs the clips of any number of reference batches as one [B, L] problem in which every clip carries the
 * padded length of ITS OWN batch,
 *   pad_len  int64 [B], HOST memory, read before the call returns: samples of clip b's own reference batch after padding (the
 *            longest clip of that batch), 400 <= pad_len[b] <= L.  L = the largest of them (or more).
 *   wav      f32 [B, L] device: clip b in wav[b, 0 .. pad_len[b]) exactly as its own batch would hold it (its samples, then the
 *            zeros of padding="longest"); what lies beyond pad_len[b] is never used
 *   attention_mask  i32 [B, L] device or NULL: as in loco_forward for the first pad_len[b] entries of row b; entries beyond MUST be
 *            0 (the valid-frame count is the row sum).
 *   valid_len  int64 [B] HOST or NULL: the row sums of that mask, for callers that know them -- HF reduces the mask to exactly this
 *            number before anything else (modeling_speecht5.py:569-582: attention_mask.cumsum(-1)[:, -1]), so a mask made by
 *            padding="longest" carries no other information; 0 <= valid_len[b] <= pad_len[b].  With valid_len no mask crosses
 *            PCIe and none is counted on the device.  Give one of the two, or neither = every sample below pad_len[b] is present.
 * and per clip b, with T_b = loco_output_frames(pad_len[b]) and T = loco_output_frames(L):
 *   - GroupNorm moments of conv layer 0 over the conv frames of pad_len[b] samples -- the zero tail of its own batch counts,
 *     nothing beyond (the same fp64 partial sums in the same order as a forward of that batch alone);
 *   - the positional conv reads zeros from frame T_b on; sinusoid positions 2.. for valid frames, the pad row from there on;
 *   - keys >= its valid frames are masked in attention (so are all keys >= T_b);
 *   - out[b, t, :] for t < T_b is what loco_forward gives for clip b inside its own batch, including that batch's padded frames
 *     (the reference pickles them); rows T_b <= t < T are unspecified (finite).  out_frames[b] = valid frames, as loco_forward.
 * Every other operation of the path is row-wise (GEMM rows, LayerNorm) and runs over all B * T rows at once.  A pack therefore
 * differs from the one-batch forwards it replaces by the fp32 SUMMATION ORDER OF THE GEMMS ONLY (small problems cut K into
 * slices, loco_set_precision above): <= 5e-6 relative L2, every other step is the same arithmetic in the same order.
 * Any set of reference batches may share a pack (sorting batches by length before packing minimises the rows T_b..T).
 * status / precision / workspace / concurrency exactly as loco_forward_async (loco_workspace_bytes(enc, B, L) bytes; the status
 * block also stages the per-clip lengths: it must stay untouched -- and should be pinned -- until `stream` has completed the
 * forward).  B <= loco_max_pack_clips(). */
int loco_max_pack_clips(void);
int loco_forward_packed(loco_encoder* enc, int precision, const float* wav, const int32_t* attention_mask, const int64_t* valid_len,
                        int32_t B, int64_t L, const int64_t* pad_len, float* out, int32_t* out_frames, float* const* hidden_states,
                        void* workspace, size_t workspace_bytes, void* stream, void* status);
int loco_status_range(const void* status, int32_t stage, float* amax, int32_t* layer, char* name, size_t namelen);

/* ---- sample-rate conversion to 16 kHz ("next" row f-4) ---------------------------------------------------------------------
 * The reference resamples every file on the host with librosa.load(path, sr=16000)
 * (/root/reference/speech_text/extract_speecht5_base_embeddings_slurp.py:56; librosa 0.10.0.post2 -> soxr 0.3.5 'soxr_hq',
 * requirements.txt:63,138).  soxr's source is not part of the reference, so what is implemented is its published 'HQ'
 * specification -- linear phase, pass band to 0.913 of the lower Nyquist frequency, stop band from 1.0, >= 120 dB -- as one
 * Kaiser-windowed-sinc polyphase filter with librosa's output length ceil(n * 16000 / sr_in).  PARITY UNPINNED against
 * librosa itself (expected agreement ~1e-5 relative: the two designs' ripple); pinned against an fp64 restatement of this
 * specification and design-independent properties (tests/test_gpu_resample.py).
 *   loco_resample_design  up/down = 16000/sr_in in lowest terms, taps per phase (multiple of 4); with taps_host != NULL also
 *                         writes the [up][taps_per_phase] fp32 table to HOST memory (designed in fp64; upload it once per rate)
 *   loco_resample_length  ceil(n_in * up / down)
 *   loco_op_resample      y[b, n] for n < n_out <= loco_resample_length(n_in); x f32 [B, x_stride >= n_in], zero-extended
 *                         beyond both ends; taps_dev = the table in device memory (16-byte aligned); HBM-bound, one launch. */
int loco_resample_design(int32_t sr_in, int32_t sr_out, int32_t* up, int32_t* down, int32_t* taps_per_phase, float* taps_host);
int64_t loco_resample_length(int64_t n_in, int32_t up, int32_t down);
int loco_op_resample(const float* x, int32_t B, int64_t n_in, int64_t x_stride, const float* taps_dev, int32_t up, int32_t down,
                     int32_t taps_per_phase, float* y, int64_t n_out, int64_t y_stride, void* stream);

/* ---- FLAC decoding (row a2: the corpus side of librosa.load) --------------------------------------------------------------------
 * SLURP's recordings are FLAC files; the reference reads them through librosa.load(path, sr=16000)
 * (/root/reference/speech_text/extract_speecht5_base_embeddings_slurp.py:56 -> soundfile -> libsndfile -> libFLAC), none of which is
 * needed here: loco_flac_decode is a host-side decoder of the format (RFC 9639: STREAMINFO, frame CRC-8 / CRC-16, CONSTANT / VERBATIM /
 * FIXED / LPC subframes, partitioned Rice residuals with escape, wasted bits, left-side / side-right / mid-side stereo, 4-32 bits per
 * sample), bit-exact by construction -- with verify_md5 != 0 the MD5 signature every encoder stores in STREAMINFO is checked against the
 * decoded samples, so each real file is its own known-answer test.  All pointers are HOST memory.
 *   loco_flac_info    sample rate, channels, bits per sample, total samples per channel (0 = unknown: decode with enough capacity)
 *   loco_flac_decode  mono  float32 [n] = mean over channels of sample / 2^(bits-1) (what soundfile.read(dtype="float32").mean(axis=1)
 *                     gives the reference), and / or pcm int32 [n, channels] interleaved; either may be NULL; capacity in samples per
 *                     channel; *n_samples = samples decoded.  LOCO_E_INVALID (message: loco_flac_last_error) for a malformed stream, a
 *                     CRC or MD5 mismatch; LOCO_E_WORKSPACE when capacity is too small.
 * The bytes are untrusted input: every length is checked against nbytes, a frame is parsed before its CRC-16 can be verified and a
 * crafted file carries valid CRCs anyway, so sample arithmetic wraps instead of overflowing, residuals wider than 32 bits and wasted-bit
 * counts >= the sample size are refused (tests/test_flac_sanitized.py: ~4 500 damaged streams through an ASan + UBSan build). */
const char* loco_flac_last_error(void);
int loco_flac_info(const void* data, size_t nbytes, int32_t* sample_rate, int32_t* channels, int32_t* bits_per_sample, int64_t* total_samples);
int loco_flac_decode(const void* data, size_t nbytes, float* mono, int32_t* pcm, int64_t capacity, int64_t* n_samples, int32_t verify_md5);

/* ---- waveform normaliser ("next" row f-4): SpeechT5FeatureExtractor(do_normalize=True) on the device -------------------
 * HF feature_extraction_speecht5.py:119-138 (the reference's collate_fn reaches it through processor(audio=...),
 * /root/reference/speech_text/extract_speecht5_base_embeddings_slurp.py:60): per clip, over its UNPADDED samples
 * n = sum(attention_mask[b]) (all L when the mask is NULL), y = (x - mean) / sqrt(var + 1e-7) with the population
 * variance; samples t >= n are set to padding_value.  fp64 moments in a fixed order (reproducible); out may alias wav. */
size_t loco_normalize_scratch_bytes(int32_t B);
int loco_op_normalize_waveform(const float* wav, const int32_t* attention_mask, int32_t B, int64_t L, float padding_value,
                               float* out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- text front end ("next" row f-4): SpeechT5EncoderWithTextPrenet ---------------------------------------------
 * The reference's text branch (/root/reference/speech_text/extract_speecht5_base_embeddings_slurp.py:79-93) runs
 * `model.speecht5.encoder(texts.input_ids)`: SpeechT5TextEncoderPrenet (HF modeling_speecht5.py: embed_tokens +
 * SpeechT5ScaledPositionalEncoding, x + alpha * pe[:T]) followed by the SAME 12-layer wrapped_encoder as the speech path.
 * Weights: loco_set_weight keys "text_prenet.embed_tokens.weight" [vocab,768], "text_prenet.encode_positions.alpha" (one
 * element, shape [1]) and optionally "text_prenet.encode_positions.pe" ([rows,768] or [1,rows,768]: HF's table, so that
 * positions are bit-identical; without it the library generates 1024 rows).  A handle may carry the speech prenet, the
 * text prenet, or both; loco_missing_weights does not ask for the speech prenet of a text-only handle.
 *   input_ids      [B, T] int32 token ids in [0, vocab) (device)
 *   attention_mask [B, T] int32 1 = token, 0 = right padding, or NULL (the reference passes none: pads attend like tokens)
 *   out            [B, T, 768] fp32; out_frames [B] (valid tokens) or NULL; hidden_states as loco_forward
 *   T <= loco_text_max_positions(enc) (HF: max_text_positions) */
size_t loco_text_workspace_bytes(const loco_encoder* enc, int32_t B, int32_t T);
int loco_text_max_positions(const loco_encoder* enc);
int loco_forward_text(loco_encoder* enc, const int32_t* input_ids, const int32_t* attention_mask, int32_t B, int32_t T,
                      float* out, int32_t* out_frames, float* const* hidden_states, void* workspace, size_t workspace_bytes,
                      void* stream);
/* the text forward with its own status block, as loco_forward_async is to loco_forward (several batches of transcripts in flight) */
int loco_forward_text_async(loco_encoder* enc, int precision, const int32_t* input_ids, const int32_t* attention_mask, int32_t B,
                            int32_t T, float* out, int32_t* out_frames, float* const* hidden_states, void* workspace,
                            size_t workspace_bytes, void* stream, void* status);

/* Arithmetic of the contractions (conv layers 1-6, feature projection, positional conv, QKV / out / FFN projections, Qp table,
 * QK^T, PV).  LOCO_PRECISION_MODES lists every mode loco_set_precision accepts (tests/test_cabi_symbols.py keeps the two in step):
 *   1  "f16x3" (default): operands split into fp16 hi + lo, three fp16 MFMAs (v_mfma_f32_16x16x32_f16 / 32x32x16_f16) per
 *      product, fp32 accumulate; fp32-class accuracy (embeddings 1.3e-6 relative L2 of an fp64 evaluation, <= 2e-5 on every
 *      golden) at 2.5x the speed of mode 0; numeric range guarded as described above
 *   0  "f32": exact fp32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32): 2.3e-6; no range limit beyond fp32's own
 *   2  "f16x2" (opt-in): the weights of the projection / conv GEMMs rounded to fp16 after their per-tensor power-of-two scale
 *      (the A_hi W_lo term is dropped; activations stay hi + lo, attention keeps three terms): 1.17x the speed of mode 1 at
 *      ~9e-4 relative L2 on the goldens.  That is AT north_star's 1e-3 bar, not inside it with margin: this mode DOES NOT
 *      GUARANTEE 1e-3 on other weights or inputs, is never the default and never what bench.py's `value` reports.
 * Statistics, softmax, residual streams and accumulators are fp32 in every mode.  Takes effect at the next loco_forward.
 * Determinism: for a given batch shape [B, L] and mode the output is bitwise reproducible.  The summation ORDER of the GEMMs
 * depends on that shape -- small problems (B*T <= 8192 frames) cut K into slices whose count follows from (B*T, N, K) -- so
 * the same clip in batches of different total size agrees to fp32 rounding (<= 4e-6), not bitwise; batch composition is part
 * of the reference's function anyway (GroupNorm over the padded axis). */
#define LOCO_PRECISION_MODES "0 f32, 1 f16x3, 2 f16x2"
const char* loco_precision_name(int mode); /* "f32" / "f16x3" / "f16x2"; NULL for a mode loco_set_precision rejects (host only) */
int loco_set_precision(loco_encoder* enc, int mode);
int loco_get_precision(const loco_encoder* enc);

/* Concurrency inside one loco_forward.  n = 2 (default): a batch whose halves each hold >= 1024 frames runs as two
 * half-batches, the second on a stream the encoder owns, forked from and joined back to `stream` with events (so the
 * call still behaves as one in-order operation on `stream`, also under stream capture).  Clips are independent, so the
 * output is bit-identical to n = 1 for halves of more than 8192 frames, and equal up to the fp32 summation order of the
 * split-K GEMM path (<= 4e-6 relative, still run-to-run deterministic) below that; the gain (2-8 %, largest for mid-size batches) is the other half's kernels filling
 * each kernel's last, partly filled round of workgroups.  loco_workspace_bytes covers both modes.  Profiling, hidden states and taps use n = 1. */
int loco_set_streams(loco_encoder* enc, int n);

/* Stage taps for parity tests: when set (device pointers, may individually be NULL) the next forwards also
 * copy the conv-stack output [B,T,512], the feature projection [B,T,768] and the prenet output [B,T,768]. */
int loco_set_taps(loco_encoder* enc, float* conv_stack, float* feature_projection, float* prenet);

/* Attention probabilities (HF output_attentions=True, modeling:930-955).  probs: NULL (unbind), or a host array of n == layers
 * device pointers, each to fp32 [B,12,T,T] for the batch of the next forward.  Like the taps, a binding stays until it is
 * cleared: every loco_forward, loco_forward_checked and loco_forward_text of the handle fills it, layer l right after layer l's
 * attention launch (one attention_probs kernel per layer), with
 *   P[b,h,i,j] = softmax_j(q_i . k_j + qp[i, clip(i-j)+160]) over the valid keys j < frames[b],  P[b,h,i,j] = 0 exactly for
 *   j >= frames[b];  padded query rows are written too (a softmax over the valid keys, as HF writes them).
 * Memory: layers * B * 12 * T^2 * 4 bytes (12 layers of 30 s x 8: 10.3 GB).  While a binding is set, forwards take the single
 * in-order pass (as hidden states and taps), a range fallback of loco_forward_checked overwrites the buffers with the exact-fp32
 * re-run, and loco_forward_async, loco_forward_packed and loco_forward_text_async return LOCO_E_STATE.  n != layers:
 * LOCO_E_INVALID.  The default path (nothing bound) launches no extra kernel. */
int loco_set_attention_outputs(loco_encoder* enc, float* const* probs, int32_t n);

/* ---- per-kernel timing (bench.py's roofline leg) --------------------------------------------------
 * With profiling on, every kernel launch inside loco_forward is bracketed by hipEvents recorded on the
 * launch stream.  loco_profile_read synchronises those events and returns per-kernel totals since the
 * last loco_profile_reset. */
typedef struct loco_kernel_stat {
    char name[48];
    int64_t launches;
    double ms;    /* sum of launch durations */
    double flops; /* algorithmic FLOPs (2*MAC) of those launches */
    double bytes; /* algorithmic bytes (compulsory reads + writes) of those launches */
} loco_kernel_stat;

int loco_set_profiling(loco_encoder* enc, int on);
/* Bracket only the launches of ONE bucket (a loco_kernel_stat name, e.g. "gemm_f16x3"); NULL or "" = all of them again.  Two event
 * records per launch cost ~1 ms of a 52 ms forward when every launch carries them: bench.py times its steps with events on the
 * dominant bucket only and takes the per-kernel table from its warm-up steps. */
int loco_set_profiling_filter(loco_encoder* enc, const char* bucket);
int loco_profile_reset(loco_encoder* enc);
int loco_profile_read(loco_encoder* enc, loco_kernel_stat* stats, int max_stats); /* returns count */

/* ---- single operators (used by the parity tests; same kernels loco_forward launches) --------------- */

/* y[r,:] = LayerNorm(x[r,:]) * gamma + beta; dim in {512, 768}; y may alias x.  (modeling:501,1023,1025,1276) */
int loco_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int32_t dim,
                      float eps, void* stream);

/* C[z][m,n] = epi(sum_k A[z][m*lda+k] * W[n*ldw+k] + bias[n]) (+ R[z][m*ldr+n]); fp32 MFMA.
 * epilogue: 0 = none, 1 = exact-erf GELU, 2 = add residual R, 5 = tanh GELU (GPT-2's gelu_new).  K % 32 == 0; lda/ldw/ldc/ldr % 4 == 0.
 * z = z1*nb2 + z2 walks nb1*nb2 problems with element strides (sA1,sA2), (sC1,sC2) (R uses C's). */
int loco_op_gemm(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, const float* R, int64_t ldr,
                 float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t nb1, int32_t nb2,
                 int64_t sA1, int64_t sA2, int64_t sC1, int64_t sC2, void* stream);

/* conv layer 0: Conv1d(1->512,k=10,s=5,no bias) + GroupNorm(512 groups, stats over the whole padded time
 * axis) + GELU, channels-last output [B, T0, 512], T0 = (L-10)/5+1.  (modeling:260-281)
 * w [512,10], gn_w/gn_b [512]; scratch >= loco_conv0_scratch_bytes(B). */
size_t loco_conv0_scratch_bytes(int32_t B);
int loco_op_conv0_gn_gelu(const float* wav, int32_t B, int64_t L, const float* w, const float* gn_w, const float* gn_b,
                          float* out, void* scratch, void* stream);

/* The same layer with every output form the forward uses.  Exactly one of `out` (fp32 [B, T0, 512]) and the pair out_hi / out_lo
 * (fp16 planes [B, T0, 512], hi = fp16(v), lo = fp16(v - hi)) is non-null, else LOCO_E_INVALID; with `out` the result has the bits of
 * loco_op_conv0_gn_gelu.  range_slot (may be NULL, read only with planes): 8 fp32 words, word i raised -- never lowered -- to
 * max |v| over the 64-frame blocks i, i + 8, ... of every clip, as an unsigned maximum of the bit patterns.
 * t0_clip (device int32 [B], may be NULL; 1 <= t0_clip[b] <= T0): the packed forward's promise.  Clip b's GroupNorm statistics run
 * over its first t0_clip[b] conv frames only, summed in the order a launch of that clip alone, at a length whose T0 is t0_clip[b],
 * would sum them: frames t < t0_clip[b] have that launch's bits.  Frames t >= t0_clip[b] are written as +0.0 (zero bits in both
 * planes) and enter the range words as 0. */
int loco_op_conv0_gn_gelu_ex(const float* wav, int32_t B, int64_t L, const float* w, const float* gn_w, const float* gn_b,
                             float* out, void* out_hi, void* out_lo, float* range_slot, const int32_t* t0_clip, void* scratch,
                             void* stream);

/* frames[b] = loco_output_frames(sum(mask[b,:])); mask NULL -> loco_output_frames(L). (modeling:569-598) */
int loco_op_frame_counts(const int32_t* mask, int32_t B, int64_t L, int32_t* frames, void* stream);

/* positional conv embedding + sinusoidal positions (modeling:389-397,555-564):
 *   out = h + GELU(groupedconv(h) + bias) + sin_table[pos], pos = t+2 for t < frames[b] else 1.
 * h,out [B,T,768]; w_folded [16][128][48][48] (group, tap, out, in) = weight-norm already applied;
 * sin_table [rows,768] with rows >= T+2; frames NULL = all valid. */
int loco_op_pos_conv(const float* h, const float* w_folded, const float* bias, const float* sin_table, const int32_t* frames,
                     float* out, int32_t B, int32_t T, void* stream);

/* self-attention core (modeling:911-982): qkv [B,T,2304] = [q*1/8 | k | v] per frame, qp [B,12,T,320] =
 * q_scaled . pe_k^T, frames [B] or NULL; ctx [B,T,768] = softmax(q k^T + qp[i, clip(i-j)+160] + mask) v,
 * heads merged.  Flash-style: no [T,T] tensor is ever formed.
 * What the launch reads of clip b, with n = frames[b] (T where frames is NULL or frames[b] is <= 0 or > T): rows [0, R) of k and v,
 * R = min(T, 64 * ceil(n / 64)), and nothing of rows [R, T).  Keys [n, R) are masked by a select, so their k rows and table entries
 * may hold anything, NaN included; their probabilities are exactly zero but still multiply v, so rows [n, R) of v MUST BE FINITE
 * (0 * NaN and 0 * inf are NaN).  Every row of ctx below T is written, padded query rows included; nothing else is. */
int loco_op_attention(const float* qkv, const float* qp, const int32_t* frames, float* ctx, int32_t B, int32_t T,
                      void* stream);
/* The probabilities of that attention (attention_probs.hip): probs [B,12,T,T] fp32 as loco_set_attention_outputs describes,
 * qkv / qp / frames as loco_op_attention (frames NULL: every key valid).  Exact-fp32 products.
 * What the launch reads of clip b, with n = frames[b] (T where frames is NULL or frames[b] is <= 0 or > T): every q row [0, T), padded
 * queries included; k rows [0, R), R = min(T, 32 * ceil(n / 32)), of which rows [n, R) are discarded by a select and may hold anything,
 * NaN included, and nothing of k rows [R, T); no v.  Of table row i: for i < n + 158 exactly the entries its valid keys j < n select,
 * columns clip(i - n + 1) + 160 ... clip(i) + 160 with clip(x) = min(max(x, -160), 159); for i >= n + 158 (every valid key is 159 or more
 * frames in the past and would read column 319) NO entry: a bias that is constant over a row cancels in the softmax, and the kernel adds
 * 0 there.  A masked key reads no entry.  Every probs[b, h, i < T, j < T] is written -- masked keys j >= n as +0.0f -- and nothing else.
 * Scores are expected finite: a +-inf or NaN among the entries or products a valid key reads is outside the contract (NaN rows). */
int loco_op_attention_probs(const float* qkv, const float* qp, const int32_t* frames, float* probs, int32_t B, int32_t T,
                            void* stream);

/* ---- split-precision ("f16x3") operators: fp32-class accuracy at the fp16 matrix-core rate ----------------------
 * x = hi + lo with hi = fp16(x), lo = fp16(x - hi); A W^T ~= Ahi Whi^T + Alo Whi^T + Ahi Wlo^T (gemm_f16x3.hip). */
int loco_op_split_f16(const float* x, void* hi, void* lo, int64_t n, void* stream); /* n % 4 == 0 */
/* as loco_op_gemm with fp16 hi/lo planes for A and W (lda/ldw % 8 == 0); output fp32 C, or split planes Chi/Clo
 * when Chi != NULL (the form the next GEMM consumes).  Plane outputs are written as 16-byte pieces: with Chi set, ldc, sC1 and
 * sC2 must be multiples of 8 halves (fp32 output: of 4 floats); anything else is LOCO_E_INVALID. */
int loco_op_gemm_f16x3(const void* Ahi, const void* Alo, int64_t lda, const void* Whi, const void* Wlo, int64_t ldw,
                       const float* bias, const float* R, int64_t ldr, float* C, void* Chi, void* Clo, int64_t ldc,
                       int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t nb1, int32_t nb2, int64_t sA1, int64_t sA2,
                       int64_t sC1, int64_t sC2, void* stream);

/* A convolution layer (kernel = taps <= 3, any stride: lda = stride * Cin) as the same GEMM over overlapping input rows, the way
 * loco_forward runs feature_encoder.conv_layers.1-6: A = input planes [B][Tin][Cin] (sA1 = Tin * Cin), output [B][Tout][N], and the
 * k axis walked (64-channel block, tap slot, 32-channel half) with tap slots 0, 2, 1 -- so that the two uses of an input row shared
 * by neighbouring outputs, and the two halves of every 128-byte line, are a k-tile or two apart and the row is fetched from HBM once.
 * The weight planes must be in that order: loco_op_permute_conv_k turns [N][taps][Cin] (tap-major K, fp32) into
 * [N][Cin/64][slot][2][32]; split it with loco_op_split_f16.  Cin % 64 == 0. */
int loco_op_permute_conv_k(const float* w, float* out, int32_t N, int32_t taps, int32_t Cin, void* stream);
int loco_op_conv_gemm_f16x3(const void* Ahi, const void* Alo, int64_t lda, const void* Whi, const void* Wlo, float* C, void* Chi,
                            void* Clo, int32_t Tout, int32_t N, int32_t Cin, int32_t taps, int32_t epilogue, int32_t B, int64_t sA1,
                            void* stream);

/* The same GEMM with the split-K workspace loco_forward hands it for small problems (M <= 512 and a grid that cannot
 * fill the chip): K is cut into slices computed side by side, partial sums (fp32, >= loco_gemm_splitk_bytes()) are added in
 * a fixed order by a second kernel that applies the epilogue.  Larger problems ignore the workspace. */
size_t loco_gemm_splitk_bytes(void);
/* diagnostics: re-read the LOCO_GEMM_* A/B knobs (tile form, persistence, ...) and LOCO_ATTN_LONG (0 / 1: force the attention
 * instantiation without / with the long-sequence rescale skip) from the environment; they are otherwise read once */
void loco_debug_reload_gemm_knobs(void);
int loco_op_gemm_f16x3_splitk(const void* Ahi, const void* Alo, int64_t lda, const void* Whi, const void* Wlo, int64_t ldw,
                              const float* bias, const float* R, int64_t ldr, float* C, void* Chi, void* Clo, int64_t ldc,
                              int32_t M, int32_t N, int32_t K, int32_t epilogue, void* splitk_ws, size_t splitk_bytes,
                              void* stream);

/* Every argument of the split-precision GEMM as loco_forward launches it (parity tests): those of loco_op_gemm_f16x3 plus
 *   Rhi / Rlo    epilogue 2: the residual as fp16 hi/lo planes (element offsets and ldr of R, ldr % 8 == 0) instead of R;
 *   out_scale    the accumulator is multiplied by it before bias / epilogue (weight planes holding W * 2^k: out_scale = 2^-k);
 *   terms        3, or 2 = the A_hi W_lo term dropped (precision mode "f16x2");
 *   range_slot   device, 8 floats, or NULL: max|x| of what is written into planes is folded into max(range_slot[0..7]);
 *   qkv_stride   epilogue 3 (q|k|v scatter; N = 2304, one batch entry, plane output): columns [768 j, 768 j + 768) go to rows of 768
 *                halves at Chi / Clo + j * qkv_stride; qkv_stride >= M * 768 and % 8 == 0;
 *   splitk_ws    NULL, or the workspace of loco_op_gemm_f16x3_splitk (splitk_bytes >= loco_gemm_splitk_bytes());
 *   co_scheduled nonzero: the tile choice stops rounding up to whole rounds of workgroups (the two half-batch schedule).
 * struct_size must be sizeof(LocoGemmF16Desc). */
typedef struct LocoGemmF16Desc {
    uint32_t struct_size;
    int32_t M, N, K, epilogue, nb1, nb2, terms, co_scheduled;
    const void *Ahi, *Alo, *Whi, *Wlo;
    const float *bias, *R;
    const void *Rhi, *Rlo;
    float* C;
    void *Chi, *Clo;
    float* range_slot;
    void* splitk_ws;
    size_t splitk_bytes;
    int64_t lda, ldw, ldc, ldr, sA1, sA2, sC1, sC2, qkv_stride;
    float out_scale;
} LocoGemmF16Desc;
int loco_op_gemm_f16x3_desc(const LocoGemmF16Desc* desc, void* stream);

/* The grouped positional conv of the f16x3 forward (gemm_f16x3.hip), as loco_forward runs it: h [B,T,768] is re-laid into group-major
 * fp16 planes with a 64-frame zero halo (ghi / glo: B * 16 * (T + 128) * 48 halves each; rows t >= rows_clip[b] read as zeros when
 * rows_clip is given), then out = h + GELU(out_scale * conv + bias) + sin_table[pos] as loco_op_pos_conv.  whi / wlo: planes of the
 * folded weight in GEMM order [16][48][128 * 48] ([g][o][tap * 48 + i]) times 1 / out_scale (a power of two); terms 3 or 2;
 * splitk_ws NULL or >= loco_gemm_splitk_bytes() (taken for B * 16 * ceil(T / 512) <= 64). */
int loco_op_pos_conv_f16x3(const float* h, const void* whi, const void* wlo, const float* bias, const float* sin_table,
                           const int32_t* frames, const int32_t* rows_clip, float out_scale, int32_t terms, void* ghi, void* glo,
                           void* splitk_ws, size_t splitk_bytes, float* out, int32_t B, int32_t T, void* stream);

/* loco_op_layernorm as the f16x3 forward runs it: y (optional fp32 copy), yhi = fp16(y) and ylo = fp16(y - yhi) as planes
 * [rows, dim], and nonfinite_slot (device, 8 floats, or NULL) set to +inf when a row's statistics are not finite. */
int loco_op_layernorm_f16x3(const float* x, const float* gamma, const float* beta, float* y, void* yhi, void* ylo,
                            float* nonfinite_slot, int64_t rows, int32_t dim, float eps, void* stream);
/* The LayerNorm behind the out-projection and the second FFN GEMM of the f16x3 forward: loco_op_layernorm_f16x3 of
 * x + (rhi + rlo), a residual given as fp16 hi/lo planes [rows, dim] (8-byte aligned, both required).  The sum is formed in fp32,
 * hi + lo first, before the row's mean: the bits of loco_op_layernorm_f16x3 on that sum. */
int loco_op_layernorm_f16x3_residual(const float* x, const void* rhi, const void* rlo, const float* gamma, const float* beta,
                                     float* y, void* yhi, void* ylo, float* nonfinite_slot, int64_t rows, int32_t dim,
                                     float eps, void* stream);

/* split-precision attention core: q, k and v as fp16 hi/lo planes [B*T,768] (q pre-scaled by 1/8) -- the layout the fused q|k|v
 * projection writes; the kernel transposes its V tiles with the LDS read; qp/frames/ctx as loco_op_attention, and the same contract
 * for what is read: rows [0, min(T, 64 * ceil(frames[b] / 64))) of the k and v planes of clip b, of which the v rows from frames[b]
 * on must be finite in both planes (they are multiplied by a zero probability); the k rows there may hold anything. */
int loco_op_attention_f16x3(const void* qhi, const void* qlo, const void* khi, const void* klo, const void* vhi,
                            const void* vlo, const float* qp, const int32_t* frames, float* ctx, int32_t B, int32_t T,
                            void* stream);
/* The form loco_forward runs: the relative-position table qp[b, head, i, 0..319] = q_scaled[i] . pe_k^T * pe_scale is computed by the
 * attention kernel itself (each wave for its own 32 queries) from pe_k as fp16 hi/lo planes [320][64] -- no table GEMM in front
 * of it -- into qp_scratch ([B,12,T,320] fp32: written and read back by the launch).  Only the 32-column blocks some key can read
 * are formed: afterwards row i of qp_scratch holds columns 32 * floor((lo + 160) / 32) ... 32 * floor((hi + 160) / 32) + 31 with
 * lo = max(i0 - (64 * ceil(frames / 64) - 1), -160), hi = min(i0 + 31, 159), i0 = 32 * floor(i / 32); its other entries are untouched.
 * lo has no upper clamp: for i0 >= 64 * ceil(frames / 64) + 159 (padded queries at least 159 frames behind the end of the last key
 * tile: T >= 225) lo >= 160, the range is empty and the row's 320 entries are ALL untouched.  Every key of such a wave is past-clipped;
 * it uses 0 for their common bias (c_past) in place of entry 319, which changes no probability of the row: the context is that of
 * the true table.  A consumer of qp_scratch must not read those rows (loco_op_attention_probs_f16x3 does not).
 * k and v rows as loco_op_attention_f16x3: v rows from frames[b] up to min(T, 64 * ceil(frames[b] / 64)) must be finite. */
int loco_op_attention_f16x3_pe(const void* qhi, const void* qlo, const void* khi, const void* klo, const void* vhi, const void* vlo,
                               const void* pe_hi, const void* pe_lo, float pe_scale, float* qp_scratch, const int32_t* frames,
                               float* ctx, int32_t B, int32_t T, void* stream);
/* The instantiations loco_forward launches: the context leaves as fp16 hi/lo planes ctx_hi / ctx_lo [B*T,768] (hi = fp16(x), lo =
 * fp16(x - hi), bit for bit what loco_op_split_f16 makes of the fp32 context of the two entries above), the A operand of the
 * out-projection GEMM.  pe_hi and pe_lo both NULL: qp is the input table of loco_op_attention_f16x3; both given: qp is the scratch
 * of loco_op_attention_f16x3_pe, filled by the launch.  Exactly one of them, or any other pointer NULL: LOCO_E_INVALID.  The same
 * contract for k and v rows: v rows from frames[b] up to min(T, 64 * ceil(frames[b] / 64)) must be finite. */
int loco_op_attention_f16x3_planes(const void* qhi, const void* qlo, const void* khi, const void* klo, const void* vhi, const void* vlo,
                                   const void* pe_hi, const void* pe_lo, float pe_scale, float* qp, const int32_t* frames,
                                   void* ctx_hi, void* ctx_lo, int32_t B, int32_t T, void* stream);
/* loco_op_attention_probs on fp16 hi/lo planes of q (pre-scaled) and k, [B*T,768] each, as the QKV projection writes them: terms 3
 * (Qlo Khi + Qhi Klo + Qhi Khi) or 2 (the Klo term dropped) v_mfma_f32_32x32x16_f16 per product.  Reads and writes exactly what
 * loco_op_attention_probs does, in both planes: q rows [0, T), k rows [0, min(T, 32 * ceil(n / 32))), and of table row i the entries
 * clip(i - n + 1) + 160 ... clip(i) + 160 for i < n + 158, none for i >= n + 158, none for a masked key.  qp may therefore be the
 * qp_scratch a loco_op_attention_f16x3_pe launch with the same frames has just filled, whatever the allocation held before: every
 * entry read lies in a block that launch formed (for i < n + 158 its lo is at most i - n + 1 < 160, so the range of formed blocks is
 * not empty and covers the entries above), and the rows it leaves wholly unformed (i0 >= 64 * ceil(n / 64) + 159, all of them
 * i >= n + 158) are not read. */
int loco_op_attention_probs_f16x3(const void* qhi, const void* qlo, const void* khi, const void* klo, const float* qp,
                                  const int32_t* frames, float* probs, int32_t B, int32_t T, int32_t terms, void* stream);

/* ---- intent head: the first consumer of the embeddings ("next" row f-1) --------------------------------------
 * IntentClassifier (/root/reference/speech_text/intent_classifier.py:24-49): pooling over time
 * (method 0 = average, 1 = max, 2 = learned-query softmax attention, :32-36) + Linear(768,101), and one
 * optimisation step of train_classifier.py:104-115: soft-label CrossEntropyLoss (mean over the batch) +
 * Adam with L2 weight decay (:66-68).  Parameters are one flat fp32 vector [q (768) | W (101*768) | b (101)];
 * gradients use the same layout, so a data-parallel trainer all-reduces ONE 78 437-float buffer between
 * loco_head_loss_grad and loco_head_adam_step.  x is [B, T, 768] exactly as the reference's collate_fn pads it
 * (zeros, no mask: padded frames take part in the pooling there too, train_classifier.py:47-50). */
typedef struct loco_head loco_head;
const char* loco_head_last_error(void);
loco_head* loco_head_create(int method);
void loco_head_destroy(loco_head* head);
int32_t loco_head_num_params(void); /* 78 437 */
int loco_head_set_params(loco_head* head, const float* flat); /* host or device; resets the Adam state */
int loco_head_get_params(const loco_head* head, float* flat);
size_t loco_head_workspace_bytes(int32_t B, int32_t T);
/* logits f32 [B,101] (the reference's forward returns [B,1,101]) */
int loco_head_forward(loco_head* head, const float* x, int32_t B, int32_t T, float* logits, void* workspace,
                      size_t workspace_bytes, void* stream);
/* forward + backward: loss (device scalar), optional logits [B,101], grads [78 437] (device) */
int loco_head_loss_grad(loco_head* head, const float* x, const float* target, int32_t B, int32_t T, float* loss,
                        float* logits, float* grads, void* workspace, size_t workspace_bytes, void* stream);
/* Ragged forms: the batch is gathered on the device from a store of clips laid end to end, no padded copy.
 *   store   f32 [rows, 768]; clip i is rows offsets[i] .. offsets[i] + lengths[i] - 1 (offsets int64, in rows: a store may
 *           hold more than 2^31 floats)
 *   targets f32 [n_items, 101] (loss_grad only)
 *   idx     int32 [B] (device): batch entry b is clip idx[b]; indices may repeat and come in any order
 * Contract, NOT checked on the device: every idx[b] is in [0, n_items) and lengths[idx[b]] <= T_pad.  The batch is pooled
 * exactly as if pad_sequence had zero-padded every clip to T_pad frames: average divides by T_pad, max sees the zeros,
 * attention gives each pad frame the score 0 (it adds exp(-m) to the softmax denominator), and in the attention backward
 * pad frames add alpha_t (dp.(0 - p))(0 - p) to the query gradient.  Results are bit-identical to loco_head_forward /
 * loco_head_loss_grad on the same batch padded on the host.  Workspace: loco_head_workspace_bytes(B, T_pad).  Null pointers
 * (logits of loss_grad_ragged excepted), B <= 0 or T_pad <= 0 return LOCO_E_INVALID; a too-small workspace LOCO_E_WORKSPACE.
 * Asynchronous on stream: no synchronisation, no host allocation. */
int loco_head_forward_ragged(loco_head* head, const float* store, const int64_t* offsets, const int32_t* lengths,
                             const int32_t* idx, int32_t B, int32_t T_pad, float* logits, void* workspace,
                             size_t workspace_bytes, void* stream);
int loco_head_loss_grad_ragged(loco_head* head, const float* store, const int64_t* offsets, const int32_t* lengths,
                               const float* targets, const int32_t* idx, int32_t B, int32_t T_pad, float* loss,
                               float* logits, float* grads, void* workspace, size_t workspace_bytes, void* stream);
/* torch.optim.Adam semantics (weight decay added to the gradient, bias correction); q is left untouched for
 * methods 0/1, where the reference's q.grad is None */
int loco_head_adam_step(loco_head* head, const float* grads, float lr, float beta1, float beta2, float eps,
                        float weight_decay, void* stream);

/* ---- text decoder: SpeechT5ForSpeechToText's other half (teacher-forced logits, greedy generate) ------------------------------
 * The reference's notebooks call `model_stt.generate(**audios, max_length=100)` and `model_stt(**audios, decoder_input_ids=ids)`.
 * SpeechT5DecoderWithTextPrenet (HF modeling_speecht5.py: SpeechT5TextDecoderPrenet -- embed_tokens + sinusoid positions with
 * padding_idx 1 -- and 6 post-LN SpeechT5DecoderLayer: causal self-attention, cross-attention over the encoder output, erf-GELU
 * feed-forward) + SpeechT5TextDecoderPostnet (lm_head, no bias).  Weights go through loco_set_weight under HF's names below
 * "speecht5.": "decoder.prenet.embed_tokens.weight" [V,768], "decoder.wrapped_decoder.layers.N.{self_attn,encoder_attn}.
 * {q,k,v,out}_proj.{weight,bias}", "...layers.N.{self_attn_layer_norm,encoder_attn_layer_norm,final_layer_norm}.{weight,bias}",
 * "...layers.N.feed_forward.{intermediate_dense,output_dense}.{weight,bias}", "text_decoder_postnet.lm_head.weight" [V,768]; the
 * embedding and lm_head are tied in HF: either one suffices, both given are used as given.  Optionally
 * "decoder.prenet.embed_positions.weights" [>= 452,768] (HF's non-persistent buffer; otherwise generated).  The layer count
 * follows from the keys.  A handle without any decoder tensor behaves exactly as before; with some of them,
 * loco_missing_weights names the rest.  Every decoder product is exact fp32 in every precision mode, the cross-attention
 * k|v projection of the encoder output (M = B * T_enc, the existing fp32 MFMA GEMM) included.
 *   enc_out      f32 [B, T_enc, 768] the encoder's last_hidden_state (device); enc_frames i32 [B] valid frames per clip (device:
 *                loco_forward's out_frames) or NULL = all T_enc; cross-attention sees keys j < enc_frames[b]
 *   workspace    >= loco_decoder_workspace_bytes(enc, B, T_enc, S_max) bytes (device): cross k|v cache [B, T_enc, layers, 1536], self k|v
 *                cache [layers, B, S_max, 1536], token buffer i32 [B, S_max], per-row state, scratch.  It carries ALL state between
 *                loco_decoder_begin and the steps, so several utterance batches may be decoded side by side.
 * Limits: S, S_max, max_length <= 450 (max_text_positions) and, for begin / step / generate, B <= loco_decoder_max_batch() = 64
 * rows of the weight-streaming GEMM: LOCO_E_INVALID naming the limit.  No decoder weights: LOCO_E_STATE.
 *   loco_decoder_forward   teacher-forced: decoder_input_ids i32 [B, S] (device) -> logits f32 [B, S, V]; hidden_states NULL or a
 *                          host array of layers + 1 device pointers f32 [B, S, 768] (inputs of every layer and the last output)
 *   loco_decoder_begin     cross k|v projection, token buffer := <s> (2) then <pad>, row state reset
 *   loco_decoder_step      step t (0-based): consumes token t of every row, appends token t + 1 = argmax (lowest index wins ties), <pad>
 *                          (1) for a row that has emitted </s> (2); logits NULL or f32 [B, V] (device) receiving this step's logits.
 *                          Asynchronous, no host read, capturable (a linear chain of launches).  Steps must be enqueued in order.
 *   loco_decoder_read_tokens  enqueue copies of the token buffer [B, S_max] and the row lengths [B] (tokens up to and including </s>)
 *   loco_decoder_generate  = begin + steps + stream synchronisation, greedy search as HF's generate runs it for this model: stops when
 *                          every row has emitted </s> (the device's "rows open" word is read through pinned memory every 8 steps) or at
 *                          max_length tokens (<s> included).  tokens_out i32 [B, max_length] HOST, *out_length = the length HF returns
 *                          (columns beyond it hold <pad>), lengths_out i32 [B] HOST or NULL, step_logits NULL or f32
 *                          [max_length - 1, B, V] (device).  Single caller per handle: the pinned word the poll reads belongs to the
 *                          handle (begin / step / forward keep everything in the workspace and may run side by side).
 *   loco_has_decoder       1 when the handle holds a COMPLETE set of decoder tensors (loco_missing_weights names what a partial set lacks)
 *   loco_decoder_workspace_bytes  0 for a handle without a (complete) decoder */
int loco_has_decoder(const loco_encoder* enc);
int loco_decoder_max_batch(void);
size_t loco_decoder_workspace_bytes(const loco_encoder* enc, int32_t B, int32_t T_enc, int32_t S_max);
int loco_decoder_forward(loco_encoder* enc, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc,
                         const int32_t* decoder_input_ids, int32_t S, float* logits, float* const* hidden_states, void* workspace,
                         size_t workspace_bytes, void* stream);
int loco_decoder_begin(loco_encoder* enc, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc, int32_t S_max,
                       void* workspace, size_t workspace_bytes, void* stream);
int loco_decoder_step(loco_encoder* enc, int32_t B, int32_t T_enc, int32_t S_max, int32_t t, float* logits, void* workspace,
                      size_t workspace_bytes, void* stream);
int loco_decoder_read_tokens(const loco_encoder* enc, int32_t B, int32_t T_enc, int32_t S_max, int32_t* tokens, int32_t* lengths,
                             const void* workspace, size_t workspace_bytes, void* stream);
int loco_decoder_generate(loco_encoder* enc, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc, int32_t max_length,
                          int32_t* tokens_out, int32_t* lengths_out, int32_t* out_length, float* step_logits, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The two new kernels as operators (parity tests).  loco_op_skinny_gemm: loco_op_gemm's contract (epilogues 0 / 1 / 2, dense C) for
 * M <= 64 rows and K % 256 == 0 on the weight-streaming kernel, any N; LOCO_E_INVALID above 64 rows.  loco_op_decoder_attention:
 * q [B,Sq,768], k / v [B,Tk,768] (12 heads x 64), out [B,Sq,768] = softmax_j(scale q.k) v over keys j < key_counts[b] (NULL: Tk) and,
 * when causal != 0, j <= i + causal_offset; long key ranges are split over workgroups and merged in a fixed order (scratch >=
 * loco_decoder_attention_scratch_bytes). */
int loco_op_skinny_gemm(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, const float* R, int64_t ldr, float* C,
                        int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epilogue, void* stream);
size_t loco_decoder_attention_scratch_bytes(int32_t B, int32_t Sq, int32_t Tk);
int loco_op_decoder_attention(const float* q, const float* k, const float* v, const int32_t* key_counts, float* out, int32_t B, int32_t Sq,
                              int32_t Tk, int32_t causal, int32_t causal_offset, float scale, void* scratch, size_t scratch_bytes, void* stream);
/* The forms of those two kernels that only the decode step, the slot pool and the language model launch, as operators (per-element
 * tests).  All strides are in floats.
 *   loco_op_skinny_gemm_split: A W^T + bias (NULL: none) without an epilogue, columns [0, nsplit) to C[m ldc + n], columns [nsplit, N)
 *     to C2.  c2_rows NULL (the decode step's q | k|v product): C2[m ldc2 + n - nsplit].  c2_rows [M] on the device (the slot pool's):
 *     C2[m ldc2 + c2_rows[m] c2_row_stride + n - nsplit]; a row whose c2_rows[m] is negative writes nothing to C2.  0 <= nsplit <= N.
 *   loco_op_decoder_attention_strided: loco_op_decoder_attention with every stride the caller's: row (b, i) of q at q + b sq + i ldq,
 *     key j at k + b sk + j ldk, value j at v + b sv + j ldv, row (b, i) of out at out + b so + i ldo; head h at column 64 h of each.
 *     A query without a visible key (key_counts[b] <= 0, or causal with i + causal_offset < 0) yields zeros; key_counts[b] > Tk means Tk.
 *   loco_op_decoder_pool_attention: one query per slot (q, out [slots, 768], scale 1, not causal) over the slot's keys j < key_counts[b]
 *     at k + b sk + j ldk and values at v + b sk + j ldk; Tk_bound >= every count that is to be seen in full.  A slot's output depends
 *     on its own count and rows only, not on Tk_bound nor on the other slots.  scratch >= loco_decoder_pool_attention_scratch_bytes,
 *     1 <= slots <= 64. */
int loco_op_skinny_gemm_split(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, float* C, int64_t ldc, float* C2,
                              int64_t ldc2, const int32_t* c2_rows, int64_t c2_row_stride, int32_t nsplit, int32_t M, int32_t N, int32_t K,
                              void* stream);
int loco_op_decoder_attention_strided(const float* q, int64_t ldq, int64_t sq, const float* k, int64_t ldk, int64_t sk, const float* v, int64_t ldv,
                                      int64_t sv, const int32_t* key_counts, float* out, int64_t ldo, int64_t so, int32_t B, int32_t Sq, int32_t Tk,
                                      int32_t causal, int32_t causal_offset, float scale, void* scratch, size_t scratch_bytes, void* stream);
size_t loco_decoder_pool_attention_scratch_bytes(int32_t slots, int32_t Tk_bound);
int loco_op_decoder_pool_attention(const float* q, const float* k, int64_t ldk, int64_t sk, const float* v, const int32_t* key_counts, float* out,
                                   int32_t slots, int32_t Tk_bound, void* scratch, size_t scratch_bytes, void* stream);

/* ---- decoder slot pool: greedy decoding of a corpus, finished rows refilled -------------------------------------------------------
 * loco_decoder_generate carries every row of one batch until the longest has ended.  A pool has `slots` decoder rows that each sit at
 * their OWN position: a slot is free, open (decoding one utterance) or finished (its tokens wait to be read); a finished or free slot
 * is handed the next utterance by loco_decoder_pool_admit while the other slots go on.  An utterance's tokens and step logits are a
 * pure function of its own encoder rows, frame count and cap -- bit for bit, whichever utterances share the pool, whichever slot it
 * sits in and however the launches were sized: the cross k|v of a clip is a product of its own, and attention splits a key range at
 * fixed key indices (multiples of 256), merged in split order.  (loco_decoder_generate keeps its own split rule and its bits; the two
 * agree to the fp32 summation order, not bitwise.)
 *   workspace   >= loco_decoder_pool_workspace_bytes(enc, slots, T_cap, S_max) bytes (device): slot state (position, cap, frames,
 *               status, length), token buffer i32 [slots, S_max], cross k|v [slots, T_cap, layers, 1536], self k|v [layers, slots,
 *               S_max, 1536], row buffers and scratch.  ALL state of a pool lives there: two pools of one handle may run side by
 *               side.  Every call takes the same (slots, T_cap, S_max) the workspace was sized and initialised with.
 *   loco_decoder_pool_init   every slot free.  Must precede the first admit.
 *   loco_decoder_pool_admit  n clips into the slots slot_ids[0..n) (HOST, distinct): clip i's encoder rows are enc_out + i *
 *               clip_stride floats (device, [enc_rows[i], 768] dense rows; clip_stride % 4 == 0); enc_rows i32 [n] HOST = rows
 *               projected into the slot's cross k|v, enc_frames i32 [n] DEVICE (NULL: enc_rows) = valid frames, cross-attention sees
 *               keys j < min(enc_frames[i], enc_rows[i]) and rows beyond are never read; caps i32 [n] HOST = the utterance's own
 *               max_length (<s> included).  The slot restarts at <s>, position 0; nothing of its previous occupant is read again.
 *               Reads the slots' status back (one stream synchronisation) to refuse an open slot.
 *   loco_decoder_pool_step   one token for every open slot: slot r consumes token pos[r], writes k|v row pos[r] of its cache, attends
 *               to its keys j <= pos[r] and its frames, appends the argmax (lowest index wins ties) at pos[r] + 1 and is finished when
 *               that token is </s> (2) or pos[r] + 2 == cap[r].  Free and finished slots compute on zeros and write nothing.
 *               max_pos >= pos[r] and max_frames >= frames[r] of every open slot size the launches (host-side bounds: no device
 *               read); a slot beyond max_pos waits, keys beyond max_frames are not seen.  step_logits NULL or f32 [slots, V]
 *               (device): this step's logits, rows of slots that are not open undefined but finite.  Asynchronous, reads no host
 *               memory, a linear chain of launches.
 *   loco_decoder_pool_poll   enqueue a copy of the poll block to host_block (caller-owned, pinned): i32 [4 + 2 slots] = [slots open, 0,
 *               0, 0, status[slots] (0 free, 1 open, 2 finished), lengths[slots] (tokens written, <s> included)]
 *   loco_decoder_pool_read   enqueue a copy of slot `slot`'s token row i32 [S_max] to tokens (HOST); its first lengths[slot] entries
 *               are the utterance
 * Errors: slots > loco_decoder_max_batch(), a clip of more than T_cap rows, a cap outside 2 .. S_max, S_max outside 2 .. 450:
 * LOCO_E_INVALID naming the limit; admitting into an open slot, or a handle without decoder weights: LOCO_E_STATE; a workspace below
 * loco_decoder_pool_workspace_bytes (which is 0 for arguments outside the limits or a handle without a decoder): LOCO_E_WORKSPACE. */
size_t loco_decoder_pool_workspace_bytes(const loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max);
int loco_decoder_pool_init(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, void* workspace, size_t workspace_bytes, void* stream);
int loco_decoder_pool_admit(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t n, const int32_t* slot_ids, const float* enc_out,
                            int64_t clip_stride, const int32_t* enc_rows, const int32_t* enc_frames, const int32_t* caps, void* workspace,
                            size_t workspace_bytes, void* stream);
int loco_decoder_pool_step(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t max_pos, int32_t max_frames, float* step_logits,
                           void* workspace, size_t workspace_bytes, void* stream);
int loco_decoder_pool_poll(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t* host_block, const void* workspace,
                           size_t workspace_bytes, void* stream);
int loco_decoder_pool_read(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t slot, int32_t* tokens, const void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- decoder sampling: temperature / top-k / top-p on the device, N hypotheses per utterance in the slot pool ----------------------
 * The rule, for a row of logits l[0..V) (csrc/decoder_sample.hip, one definition):
 *   1. z_i = l_i / temperature, an fp32 division (HF's TemperatureLogitsWarper)
 *   2. top_k (0 = off, clamped to V): i survives iff fewer than top_k columns have z_j > z_i; ties at the threshold all survive
 *      (TopKLogitsWarper)
 *   3. top_p (1 = off), over the survivors with p = softmax(z) over them: A_i = the sum of p_j over survivors with z_j <= z_i; i is
 *      kept iff A_i > 1 - top_p, or i is the row's argmax (TopPLogitsWarper with min_tokens_to_keep = 1).  Equal logits are kept or
 *      dropped together.
 *   4. u = (x0 >> 8) * 2^-24 in [0, 1), x0 the first word of the Philox4x32-10 block with key (seed & 0xffffffff, seed >> 32) and
 *      counter (utterance, hypothesis, t, 0); t = the index in its token buffer of the token being written (the first sampled token
 *      has t = 1).  Nothing else feeds the generator.
 *   5. over the kept columns in ascending index, w_i = expf(z_i - max z), Z their sum: the token is the first kept index whose
 *      inclusive prefix sum exceeds u * Z, the last kept index if rounding leaves none.  The order of the additions depends on V alone;
 *      the fp32 terms of this sum and of step 3's are added in double.
 *   6. a row with a NaN, a +inf maximum or nothing but -inf: its argmax (the first NaN wins, the lowest index on a tie)
 *   7. a greedy row: the argmax of the raw logits, the token loco_decoder_pool_step appends
 * A row's token is a pure function of its V logits, the config and its counter, bit for bit.
 *   loco_op_sample_tokens   the rule alone.  logits f32 (device), row m at logits + m * ld, ld >= V, columns >= V never read;
 *               counters u32 [M, 3] (device) = (utterance, hypothesis, t) of every row; greedy NULL or i32 [M] (device), nonzero = rule 7;
 *               tokens i32 [M] (device).  For tests, each NULL or: keep i32 [M, V] (1 = the draw ran over the column; for a row of
 *               rule 6 or 7 the argmax alone), uniform f32 [M] (u of every row).  One launch, asynchronous.
 *   loco_decoder_pool_admit_samples   loco_decoder_pool_admit for n clips with `copies` hypotheses each: slot_ids i32 [n * copies]
 *               (HOST, distinct), clip i's hypotheses in slot_ids[i * copies .. (i + 1) * copies).  enc_out, clip_stride, enc_rows [n],
 *               enc_frames [n] (DEVICE or NULL), caps [n] as there, per clip.  utterances u32 [n] and hypotheses u32 [n * copies] (HOST) are
 *               the counter's first two words; greedy NULL (every slot draws) or i32 [n * copies] (HOST), nonzero = rule 7.  A clip's
 *               cross k|v is projected once, into its first slot, and copied on the device into the others: the same bytes as
 *               projected there.  One read-back of the slots' status (one stream synchronisation) per call.
 *   loco_decoder_pool_step_sample    loco_decoder_pool_step's launches with the sampling select kernel in the greedy one's place: the
 *               same bounds, end / cap / advance rules and poll block.  step_tokens NULL or i32 [slots] (device): the token each
 *               live slot appended, -100 for the others.  A slot admitted by loco_decoder_pool_admit is greedy here.
 * Which slots of a pool draw is kept by the handle, per workspace address (the greedy entry points enqueue what they always did, so
 * they cannot mark a slot on the device), from loco_decoder_pool_admit_samples until the slot is admitted again or
 * loco_decoder_pool_init runs on that workspace.  The entry (16 bytes) outlives the workspace: freeing a workspace does not tell the
 * handle, so a slot that finished still counts as drawing, and the entry goes with loco_decoder_pool_init on that address (which must
 * precede any reuse of the memory as a pool) or with loco_destroy.  The mask is an argument of the select launch, read on the host
 * when loco_decoder_pool_step_sample is called: a captured graph of that call replays the mask of the moment of capture, so admit
 * before capturing and capture again after an admission that changes which slots draw.  (utterance, hypothesis) of every slot live
 * in the workspace, after every region of a greedy pool.  loco_decoder_pool_step on a pool that holds such a slot: LOCO_E_STATE.
 * Errors: a config whose struct_size is not sizeof(loco_sample_config), a temperature that is not finite or not > 0, top_k < 0, top_p
 * outside (0, 1]: LOCO_E_INVALID naming the field; n * copies > slots and everything loco_decoder_pool_admit / _step refuse, alike. */
typedef struct loco_sample_config {
    uint32_t struct_size; /* sizeof(loco_sample_config) */
    float temperature;
    int32_t top_k;        /* 0 = off */
    float top_p;          /* 1 = off */
    uint64_t seed;
} loco_sample_config;
int loco_op_sample_tokens(const float* logits, int64_t ld, int32_t M, int32_t V, const loco_sample_config* config, const uint32_t* counters,
                          const int32_t* greedy, int32_t* tokens, int32_t* keep, float* uniform, void* stream);
int loco_decoder_pool_admit_samples(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t n, int32_t copies, const int32_t* slot_ids,
                                    const float* enc_out, int64_t clip_stride, const int32_t* enc_rows, const int32_t* enc_frames, const int32_t* caps,
                                    const uint32_t* utterances, const uint32_t* hypotheses, const int32_t* greedy, void* workspace,
                                    size_t workspace_bytes, void* stream);
int loco_decoder_pool_step_sample(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t max_pos, int32_t max_frames,
                                  const loco_sample_config* config, float* step_logits, int32_t* step_tokens, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* ---- decoder beam search: K beams per utterance in the slot pool -------------------------------------------------------------------
 * The rule (csrc/decoder_beam.hip, one definition) is HF's _beam_search with flags in place of its -1e9 sentinels, scores in double
 * and a defined tie order.  Per group: K = num_beams, V the vocabulary, cap the utterance's total length, cur the tokens every running
 * beam holds (1 at admission); running beams 0 .. K - 1 (tokens, score run[k], alive; at admission beam 0 alone is alive, score 0), a
 * finished list of at most K entries, best first, and a flag unsat (1).  One step:
 *   1. lp[k][v] = the fp32 log-softmax of row k's logits by loco_decoder_score's arithmetic; candidate (k, v) of an alive beam scores
 *      s = run[k] + (double)lp[k][v]
 *   2. the 2K best candidates by s descending, ties to the lower flat index k V + v; a NaN after every number, NaNs by index
 *   3. a candidate hits iff its token is </s> or cur + 1 >= cap
 *   4. if unsat and not (early_stopping == 1 and the list holds K): every candidate of rank < K that hits enters the list with score
 *      s / den[cur], den[n] = n ** length_penalty (a table of doubles made on the host with pow, loco_beam_den_table); the list is
 *      sorted stably (existing entries before new ones, new ones in candidate order) and cut to K
 *   5. the next running beams are the first K candidates that do not hit, in candidate order; fewer than K leave the rest not alive
 *   6. cur += 1; L = cap - 1 if early_stopping == 2 and length_penalty > 0, else cur - 1; unsat &= run[0] / den[L] > worst, worst the
 *      list's last score if it holds K, else -1e9
 *   7. the group is done when step 5 found no beam, unsat is 0, or early_stopping == 1 and the list holds K
 * Group g of a pool owns slots g K .. g K + K - 1 (slots / K groups); its K slots are open and finish together.
 *   loco_beam_den_table     den_host f64 [n] (HOST): den[i] = pow(i, length_penalty), den[0] = 1.
 *   loco_op_beam_select     the rule alone, one step for G groups on caller-supplied state, all DEVICE, rows r = g K + k:
 *               logits f32, row r at logits + r * ld, ld >= V >= 2 K; den f64 [S_max]; status, pos, cap, cur, cnt, lengths i32 [G K]
 *               (a group takes part iff status[g K] == 1 (open) and 0 <= pos[g K] < S_max - 1; pos is the index of the last token the
 *               beams hold; cur / cnt as the pool keeps them); tokens i32 and token_logprobs f32 [G K, S_max]; run f64 and alive i32
 *               [G K]; unsat and fin_count i32 [G]; fin_scores, fin_sums f64 and fin_lengths i32 [G K]; fin_tokens i32 and
 *               fin_logprobs f32 [G K, S_max].  Outputs: logprobs f32 [G K, V] (step 1's rows), parents i32 [G K] (the slot whose rows
 *               0 .. counts[r] - 1 slot r takes over: loco_op_beam_reorder's arguments), counts i32 [G K]; poll NULL or i32 [1] = slots
 *               open afterwards (G K <= 64).  A new beam's token and log-probability are written at index pos + 1 of its own row; a
 *               group that is done has status 2 and counts 0.  A group that is not open reads and writes nothing.
 *   loco_op_beam_reorder    the gather alone: buf and shadow [layers][slots][S_max][width] of 4-byte words (DEVICE, distinct); rows
 *               0 .. counts[r] - 1 of slot r become those of slot parents[r], clamped into r's group of K slots, for any mapping inside
 *               a group (the rows pass through shadow); status NULL or i32 [slots]: only slots with status 1 move.  Slots whose parent
 *               is themselves, rows >= counts[r] and other groups are not touched.  max_count >= every counts[r] sizes the launches.
 *   loco_decoder_beam_workspace_bytes   a pool's workspace with the beam regions after every region of loco_decoder_pool_workspace_bytes
 *               (which keep their offsets): shadow cache, finished lists, scores, parents, den, group state.  Initialise with
 *               loco_decoder_pool_init.
 *   loco_decoder_pool_admit_beams   n clips into the n groups group_ids (HOST, distinct, < slots / K); clip arguments as
 *               loco_decoder_pool_admit_samples (cross k|v projected once, copied K - 1 times).  One status read-back; an open group:
 *               LOCO_E_STATE.  The first call on a workspace after loco_decoder_pool_init fixes the config for that pool (kept by the
 *               handle per workspace address, as the sampling mask is); it needs every slot not open; another config later: LOCO_E_STATE.
 *   loco_decoder_pool_step_beam     loco_decoder_pool_step's launches up to the logits, then the select and reorder kernels; the same
 *               bounds.  Optional outputs (DEVICE): step_logits f32 [slots, V], step_logprobs f32 [slots, V], step_parents i32 [slots]
 *               (rows of groups that did not take part are not written).  Asynchronous, no host read.
 *   loco_decoder_pool_read_beams    group's finished list into HOST buffers (pinned for an asynchronous copy), each optional: count
 *               i32 [1], tokens i32 [K, S_max], lengths i32 [K], scores f64 [K], sum_logprobs f64 [K], token_logprobs f32 [K, S_max]
 *               (entry t = log P of token t, entry 0 = 0).  Entries >= count are not meaningful.
 * A beam pool is stepped with loco_decoder_pool_step_beam only: loco_decoder_pool_step, _step_sample, _admit and _admit_samples on it,
 * and loco_decoder_pool_step_beam on a pool that is none, return LOCO_E_STATE.
 * Errors: struct_size, num_beams outside 1 .. 16 or 2 num_beams > V, a length_penalty that is not finite, early_stopping outside 0 .. 2:
 * LOCO_E_INVALID naming the field. */
typedef struct loco_beam_config {
    uint32_t struct_size;   /* sizeof(loco_beam_config) */
    int32_t num_beams;      /* 1 .. 16 */
    double length_penalty;  /* finite */
    int32_t early_stopping; /* 0 false, 1 true, 2 "never" */
    int32_t reserved;       /* 0 */
} loco_beam_config;
int loco_beam_den_table(double length_penalty, int32_t n, double* den_host);
int loco_op_beam_select(const float* logits, int64_t ld, int32_t G, int32_t V, int32_t S_max, const loco_beam_config* config, const double* den,
                        int32_t* status, int32_t* pos, const int32_t* cap, int32_t* cur, int32_t* cnt, int32_t* lengths, int32_t* tokens,
                        float* token_logprobs, double* run, int32_t* alive, int32_t* unsat, int32_t* fin_count, double* fin_scores,
                        double* fin_sums, int32_t* fin_lengths, int32_t* fin_tokens, float* fin_logprobs, float* logprobs, int32_t* parents,
                        int32_t* counts, int32_t* poll, void* stream);
int loco_op_beam_reorder(void* buf, void* shadow, int32_t layers, int32_t slots, int32_t S_max, int64_t width, const int32_t* parents,
                         const int32_t* counts, const int32_t* status, int32_t num_beams, int32_t max_count, void* stream);
size_t loco_decoder_beam_workspace_bytes(const loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t num_beams);
int loco_decoder_pool_admit_beams(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, const loco_beam_config* config, int32_t n,
                                  const int32_t* group_ids, const float* enc_out, int64_t clip_stride, const int32_t* enc_rows,
                                  const int32_t* enc_frames, const int32_t* caps, void* workspace, size_t workspace_bytes, void* stream);
int loco_decoder_pool_step_beam(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t max_pos, int32_t max_frames,
                                float* step_logits, float* step_logprobs, int32_t* step_parents, void* workspace, size_t workspace_bytes,
                                void* stream);
int loco_decoder_pool_read_beams(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t group, int32_t* count, int32_t* tokens,
                                 int32_t* lengths, double* scores, double* sum_logprobs, float* token_logprobs, const void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---- n-gram language model over the decoder's ids, and its shallow fusion into beam search ------------------------------------------
 * The rule (csrc/ngram.hip, one definition of the chain; this project's own, pinned by a numpy restatement in tests/ngram_ref.py and
 * NOT validated against KenLM/SRILM binaries).
 * Symbols: predicted symbols are the decoder ids 0 .. V - 1; a predicted id 2 is the model's </s>.  Contexts may also hold BOS = V (the
 * model's <s>), which stands for the start token at index 0 of a row and is never predicted.
 * Model: a backoff model of order n, 1 <= n <= 8: grams g = (c_1 .. c_j, w), 0 <= j <= n - 1, each with logp[g] and bo[g] as float64
 * natural logarithms; a gram that never serves as a context has bo = 0; every w in 0 .. V - 1 has a unigram.  The one gram that ends in
 * BOS is the unigram (BOS): it carries bo of the context <s> and is never looked up as a prediction.
 * Next-token log-probability of w after a row of cur tokens: h_1 .. h_m = the row's last m = min(n - 1, cur) symbols, then
 *     acc = 0
 *     for j = m, m - 1, ..., 0:
 *         ctx = the last j symbols of h
 *         if gram (ctx, w) exists:      return acc + logp[(ctx, w)]
 *         if j > 0 and gram ctx exists: acc = acc + bo[ctx]
 * with every addition in double, in exactly this order: the device and the restatement give the same bits from the same table.
 * Fusion: step 1 of the beam rule becomes s = (run[k] + (double)lp[k][v]) + bonus[k][v], bonus[k][v] = weight * lm[k][v] + token_bonus,
 * every operation rounded once (no contraction); steps 2 - 7 are unchanged, so run, the finished sums and the finished scores carry
 * fused values, while the per-token log-probabilities stay the acoustic model's fp32 log P.  Nothing is kept per beam for the model: a
 * hypothesis' log-probabilities under it are a function of its tokens, computed afterwards by loco_op_ngram_score.
 * Limits: V <= 127, order <= 8, at most 2^26 grams -- a gram packs into one 64-bit key, 7 bits per symbol (oldest lowest) and its length
 * in bits 56 .. 59.  The table is an open-addressing hash (linear probing, load factor <= 0.5, 24 bytes per slot) in device memory.
 *   loco_ngram_create     HOST arrays: lengths i32 [n], symbols i32 [n][8] (oldest first, the predicted symbol last; entries beyond a
 *               gram's length are not read), logp f64 [n], backoff f64 [n].  Builds the table on the current device (synchronous) and
 *               returns the handle in *out.  LOCO_E_INVALID naming the gram index: a length outside 1 .. order, a symbol outside
 *               0 .. V, BOS in the predicted position of a gram of two or more symbols or anywhere but position 0 of a context, a
 *               duplicate gram, a logp or backoff that is not finite; naming the symbol: an id without a unigram; naming the field:
 *               vocab, order or n outside the limits, or no host memory for the build (28 bytes per slot, two slots per gram at least).
 *   loco_ngram_destroy    frees the table; a pool it is attached to must have been re-initialised (loco_decoder_pool_init) before.
 *   loco_op_ngram_logprobs  tokens i32 (DEVICE), row r at tokens + r * ld, ld >= S; cur i32 [R] (DEVICE): the tokens row r holds,
 *               1 .. S, index 0 the start token (read as BOS whatever its id).  out f64 [R, V] (DEVICE): the rule for every w.  One
 *               wave per row; a row's output depends on that row's tokens and the table alone.  A row whose cur is outside 1 .. S, or
 *               that holds an id outside 0 .. V - 1 among the symbols read, is NaN.  Asynchronous; no atomics, no allocation.
 *   loco_op_ngram_score   teacher-forced: tokens i32 [total] (DEVICE) hold B sequences, sequence b = tokens[starts[b] .. starts[b] +
 *               lens[b]) (starts i64 [B], lens i32 [B], DEVICE); out f64 [total]: out[starts[b] + i] = the rule for token i after
 *               tokens 0 .. i - 1 (token 0 read as BOS), 0 at i = 0.  A sequence that does not lie inside [0, total) is not touched.
 *   loco_op_beam_select_fused   loco_op_beam_select with bonus f64 [G K, V] (DEVICE) or NULL; NULL is loco_op_beam_select, bit for bit.
 *   loco_decoder_beam_fusion_workspace_bytes   loco_decoder_beam_workspace_bytes plus the bonus region, which comes after every region
 *               of it (all of which keep their offsets).
 *   loco_decoder_pool_attach_ngram   after loco_decoder_pool_init and before the pool's first loco_decoder_pool_admit_beams: the beam
 *               pool in `workspace` (at least loco_decoder_beam_fusion_workspace_bytes) fuses `lm` with `weight` and `token_bonus`.
 *               Kept by the handle per workspace address, as the beam config is, until loco_decoder_pool_init on that address.
 *               loco_decoder_pool_step_beam then launches the n-gram kernel on the pool's token rows before the select kernel; a pool
 *               with nothing attached enqueues exactly what it always did.  LOCO_E_INVALID: a model whose vocab is not the decoder's
 *               or whose table is on another device than the handle, a weight or token_bonus that is not finite; LOCO_E_STATE: a pool that has admitted groups or has a model attached. */
typedef struct loco_ngram loco_ngram;
int loco_ngram_create(int32_t vocab, int32_t order, int64_t n, const int32_t* lengths, const int32_t* symbols, const double* logp,
                      const double* backoff, loco_ngram** out);
void loco_ngram_destroy(loco_ngram* lm);
int32_t loco_ngram_vocab(const loco_ngram* lm);
int32_t loco_ngram_order(const loco_ngram* lm);
int loco_op_ngram_logprobs(const loco_ngram* lm, const int32_t* tokens, int64_t ld, int32_t S, const int32_t* cur, int32_t R, double* out,
                           void* stream);
int loco_op_ngram_score(const loco_ngram* lm, const int32_t* tokens, int64_t total, const int64_t* starts, const int32_t* lens, int32_t B,
                        double* out, void* stream);
int loco_op_beam_select_fused(const float* logits, int64_t ld, int32_t G, int32_t V, int32_t S_max, const loco_beam_config* config, const double* den,
                              int32_t* status, int32_t* pos, const int32_t* cap, int32_t* cur, int32_t* cnt, int32_t* lengths, int32_t* tokens,
                              float* token_logprobs, double* run, int32_t* alive, int32_t* unsat, int32_t* fin_count, double* fin_scores,
                              double* fin_sums, int32_t* fin_lengths, int32_t* fin_tokens, float* fin_logprobs, float* logprobs, int32_t* parents,
                              int32_t* counts, int32_t* poll, const double* bonus, void* stream);
size_t loco_decoder_beam_fusion_workspace_bytes(const loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, int32_t num_beams);
int loco_decoder_pool_attach_ngram(loco_encoder* enc, int32_t slots, int32_t T_cap, int32_t S_max, const loco_ngram* lm, double weight,
                                   double token_bonus, void* workspace, size_t workspace_bytes);

/* ---- decoder scores: log-probabilities of a transcript's tokens, per-sequence sums, the labels= loss --------------------------------
 * loco_decoder_score turns logits (loco_decoder_forward's [B, S, V], or a block of step logits) into what a transcript is judged by.
 * Stateless: no handle, no workspace.  Asynchronous, reads no host memory, two launches on `stream`; it can be captured like a step.
 *   logits         f32 (device), row m = b * S + t at logits + m * ld, ld >= V floats; columns >= V of a row are never read
 *   targets        i32 [B * S] (device) or NULL.  NULL: the target of a row is its argmax (the lowest index wins ties, the first NaN
 *                  wins: the decode step's rule).  targets[m] == ignore_index: the position does not count and its log-probability
 *                  is 0.  Another value outside [0, V) is never used as an index: the row's log-probability is NaN and it counts.
 *   token_logprobs f32 [B * S]: log_softmax(row)[target] = x[target] - max - log(sum exp(x - max)) in fp32 -- bit for bit a function
 *                  of the row's own V numbers, wherever the row sits and whatever the other rows hold.  Non-finite logits as
 *                  torch.log_softmax: -inf entries add nothing; a row that is all -inf, or holds +inf or NaN, gives NaN.
 *   chosen         NULL or i32 [B * S]: the target each row used (the argmax when targets is NULL)
 *   seq_logprob    NULL or f32 [B]: sum of sequence b's counted log-probabilities;  seq_count  NULL or i32 [B]: how many counted
 *   loss           NULL or f32 [1]: -(sum over b of the sums) / (sum over b of the counts), HF's CrossEntropyLoss() mean over the
 *                  tokens that are not ignored; NaN when none counts.  Sums are accumulated in double in an order fixed by (B, S).
 * Errors: a null logits or token_logprobs, B, S or V below 1, ld < V, B * S above 2^31 - 1: LOCO_E_INVALID. */
int loco_decoder_score(const float* logits, int64_t ld, const int32_t* targets, int32_t B, int32_t S, int32_t V, int32_t ignore_index,
                       float* token_logprobs, int32_t* chosen, float* seq_logprob, int32_t* seq_count, float* loss, void* stream);

/* ---- decoder attention probabilities and token timestamps ---------------------------------------------------------------------------
 * The decoder's attention kernels never form P (online softmax, key splits); these entry points form it with launches of their own
 * (csrc/decoder_probs.hip) beside the unchanged ones, in exact fp32 like every decoder product.
 *   loco_decoder_forward_attn   loco_decoder_forward plus self_attentions / cross_attentions: each NULL or a HOST array of `layers`
 *               device pointers, f32 [B, 12, S, S] / f32 [B, 12, S, T_enc] (HF's decoder_attentions / cross_attentions).  Self: key j
 *               is visible to query i iff j <= i (no decoder padding mask: <pad> tokens are keys like any other).  Cross: key j is
 *               visible iff j < enc_frames[b] (NULL: all T_enc).  Every other entry is written as exactly 0.0f and its key row is
 *               never read.  Logits and hidden states are bit for bit loco_decoder_forward's; with both arrays NULL the call enqueues
 *               exactly loco_decoder_forward's launches.  Same workspace and limits (S <= 450: LOCO_E_INVALID naming the limit; no
 *               decoder weights: LOCO_E_STATE).
 *   loco_decoder_align          where in the audio each token was spoken.  decoder_input_ids i32 [B, S] (device) are the labels shifted
 *               right, so that query row s predicts label s; token_counts i32 [B] (device) = n_b, the labels of row b that count (a
 *               prefix of the row).  A[b, s, t] = mean of the cross-attention P over the (layer, head) pairs in layer_heads (HOST, i32
 *               [pairs][2], distinct; NULL = every pair), accumulated in fp32 layer-major, head-minor, then multiplied by 1 / pairs.
 *               A monotone DTW over the cost -(double)A[b, s < n_b, t < F_b] (F_b = enc_frames[b], NULL: T_enc) runs in double: D[0,0] =
 *               c[0,0], D[s,t] = c[s,t] + min(D[s-1,t-1], D[s-1,t], D[s,t-1]), missing neighbours +inf, ties resolved diagonal first,
 *               then (s-1,t), then (s,t-1); one workgroup per clip.  start_frames / end_frames i32 [B, S] (device) = the first frame
 *               and the last frame + 1 of token s on the path from (n_b - 1, F_b - 1) back to (0, 0); -1 for s >= n_b (a row with
 *               n_b == 0 runs nothing).  attention: f32 [B, S, T_enc] (device) receiving A, or NULL (A stays in the workspace).
 *               workspace >= loco_decoder_align_workspace_bytes (the decoder's workspace, ONE layer's P, A, one back-pointer byte per
 *               cell).  Asynchronous; reads no device memory on the host.
 *   loco_op_decoder_attention_probs   the probabilities kernel alone: q rows at q + b sq + i ldq, key rows at k + b sk + j ldk (floats;
 *               head h at column 64 h; every stride a multiple of 4, row strides >= 768), P f32 [B, 12, Sq, Tk] dense.
 *   loco_op_dtw_align           the DTW alone on a given A (row (b, s) at A + (b S + s) ld floats, ld >= T): n i32 [B] and frames i32
 *               [B] or NULL on the device; workspace >= loco_dtw_align_workspace_bytes(B, S, T) bytes; S <= 450 (LOCO_E_INVALID). */
int loco_decoder_forward_attn(loco_encoder* enc, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc,
                              const int32_t* decoder_input_ids, int32_t S, float* logits, float* const* hidden_states,
                              float* const* self_attentions, float* const* cross_attentions, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t loco_decoder_align_workspace_bytes(const loco_encoder* enc, int32_t B, int32_t T_enc, int32_t S);
int loco_decoder_align(loco_encoder* enc, const float* enc_out, const int32_t* enc_frames, int32_t B, int32_t T_enc,
                       const int32_t* decoder_input_ids, int32_t S, const int32_t* token_counts, const int32_t* layer_heads, int32_t pairs,
                       float* attention, int32_t* start_frames, int32_t* end_frames, void* workspace, size_t workspace_bytes, void* stream);
int loco_op_decoder_attention_probs(const float* q, const float* k, const int32_t* key_counts, float* P, int32_t B, int32_t Sq, int32_t Tk,
                                    int32_t causal, int64_t ldq, int64_t sq, int64_t ldk, int64_t sk, float scale, void* stream);
size_t loco_dtw_align_workspace_bytes(int32_t B, int32_t S, int32_t T);
int loco_op_dtw_align(const float* A, int64_t ld, const int32_t* n, const int32_t* frames, int32_t B, int32_t S, int32_t T, int32_t* start,
                      int32_t* end, void* workspace, void* stream);

/* ---- long-form segmentation: a recording cut into utterance-sized pieces at pauses (csrc/segment.hip) --------------------------------
 * The decoder's rows end at 450 tokens and the model was trained on utterances of seconds, so a 10- or 60-minute recording is cut
 * before it is encoded.  PARITY UNPINNED: the reference has no counterpart; the rules are pinned by a numpy restatement
 * (tests/segment_ref.py) that agrees bit for bit on the same db array.  Frames are the encoder's: frame t covers samples
 * [320 t, 320 t + 400), F = loco_output_frames(n).  Seconds become frames by rounding s * 50 to the nearest integer, ties to even.
 *   loco_vad_default_params   the defaults of DESIGN.md 8 (struct_size set)
 *   loco_vad_frames           checks a parameter set on the host and writes frames[5] = max_frames, min_frames, min_silence, min_speech,
 *               pad.  LOCO_E_INVALID naming the field: a struct_size that is not sizeof(LocoVadParams), a value that is not finite,
 *               max_segment_s beyond LOCO_VAD_MAX_SEGMENT_S (30 s: about 15 characters a second fill the decoder's 450 positions) or
 *               below 2 frames, min_segment_s below one frame or not below max_segment_s (the walk would make no progress),
 *               min_silence_s below one frame, negative min_speech_s / pad_s / margin_db / min_dynamic_db, quantiles outside (0, 1) or
 *               noise_quantile >= peak_quantile.
 *   loco_op_frame_energy_db   db[t] = 10 log10(mean of x^2 over frame t + 1e-12) (exactly -120 for a frame of zeros), f32 [F]; one
 *               wave per frame, a fixed summation order.  n < 400: LOCO_E_INVALID.
 *   loco_op_vad_segments      ONE recording, one workgroup, nothing read back on the host.  Threshold: histogram of 0.25 dB bins from
 *               -120 dB (NaN: bin 0); noise / peak = the lower edge of the first bin whose cumulative count reaches ceil(quantile * F);
 *               peak < abs_floor_db: silent, 0 segments, *threshold_db = +inf; peak - noise < min_dynamic_db: every frame that is not
 *               NaN is speech, *threshold_db = -inf; otherwise thr = max(abs_floor_db, noise + margin_db), speech = db > thr.
 *               Clean-up: interior silence runs shorter than min_silence become speech, then speech runs shorter than min_speech become
 *               silence.  Cuts: from s = 0, the rest is the last segment when F - s <= max_frames; otherwise the next segment starts at c
 *               in (s + min_frames, s + max_frames]: the centre (a + b) / 2 of the silence run [a, b) that is longest after clipping to
 *               that window (ties: the later run), or, without one, the first frame of least db in [s + max_frames / 2, s + max_frames]
 *               (NaN counts as least).  trim: a segment loses leading and trailing silence beyond pad frames; one without a speech frame
 *               is dropped.  seg_start / seg_end i32 [max_segments] (end exclusive), *count = the number of segments, or minus that
 *               number when it exceeds max_segments (only the first max_segments are written); all outputs in device memory.
 *               workspace >= loco_vad_workspace_bytes(F) (0 for F outside 1 .. 2^24).
 *               Errors, before any launch: null pointers, F outside 1 .. 2^24, max_segments < 1, refused parameters, a workspace
 *               below loco_vad_workspace_bytes(F) (an operator's argument like any other): LOCO_E_INVALID. */
#define LOCO_VAD_MAX_SEGMENT_S 30.0
typedef struct LocoVadParams {
    uint32_t struct_size; /* sizeof(LocoVadParams) */
    int32_t trim;         /* 1 */
    double max_segment_s; /* 20 */
    double min_segment_s; /* 1 */
    double min_silence_s; /* 0.3 */
    double min_speech_s;  /* 0.1 */
    double pad_s;         /* 0.2 */
    double noise_quantile; /* 0.10 */
    double peak_quantile;  /* 0.99 */
    double margin_db;      /* 10 */
    double abs_floor_db;   /* -60 */
    double min_dynamic_db; /* 15 */
} LocoVadParams;
void loco_vad_default_params(LocoVadParams* params);
int loco_vad_frames(const LocoVadParams* params, int32_t* frames);
size_t loco_vad_workspace_bytes(int64_t F);
int loco_op_frame_energy_db(const float* wav, int64_t n, float* db, void* stream);
int loco_op_vad_segments(const float* db, int64_t F, const LocoVadParams* params, int32_t* seg_start, int32_t* seg_end, int32_t max_segments,
                         int32_t* count, float* threshold_db, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the same for a recording of C channels, one speaker per channel (a two-channel telephone call) ---------------------------------
 * Each channel is cut on its own energies, so overlapping speech stays two segments and every segment keeps its speaker side.  Telephone
 * channels leak into each other, hence a CROSS-TALK GATE at the raw-mask step.  The gate and its 15 dB default (segment.py) are this
 * project's own rule, pinned by tests/segment_channels_ref.py like the rest; they are NOT validated on real Fisher audio.
 *   loco_op_frame_energy_db_channels   wav f32 [C, stride] (n <= stride samples of each row are read) -> db f32 [C, F]; a row's bits are
 *               those of loco_op_frame_energy_db on that row.
 *   loco_op_vad_segments_channels      db f32 [C, F]; one workgroup per channel runs loco_op_vad_segments' steps on row c with one
 *               addition: mask[t] = base(t) && !(other(t) - db[c][t] > crosstalk_db), where base is the rule above (db > thr, or "not
 *               NaN" without usable silence), other(t) the maximum of db[o][t] over the channels o != c with NaN ignored (no other
 *               channel, or all NaN: not gated), the test one fp32 subtraction and a strict > (a difference of exactly crosstalk_db is
 *               kept; +inf switches the gate off).  The threshold comes from the channel's own ungated histogram.  seg_start / seg_end
 *               i32 [C, max_segments], count i32 [C], threshold_db f32 [C] as above, per channel.  overlap (may be NULL) i32
 *               [C, max_segments]: the frames of segment k of channel c in which the cleaned mask of any other channel is 1 (a silent
 *               channel's mask is all zero); one wave per segment, a second launch.  workspace >= loco_vad_channels_workspace_bytes(C, F)
 *               (0 for C outside 1 .. 8 or F outside 1 .. 2^24).
 *               Errors, before any launch, by name: null pointers (overlap excepted), C outside 1 .. 8, crosstalk_db NaN or negative,
 *               F outside 1 .. 2^24, max_segments < 1, refused parameters, a workspace that is too small: LOCO_E_INVALID. */
size_t loco_vad_channels_workspace_bytes(int32_t C, int64_t F);
int loco_op_frame_energy_db_channels(const float* wav, int32_t C, int64_t n, int64_t stride, float* db, void* stream);
int loco_op_vad_segments_channels(const float* db, int32_t C, int64_t F, const LocoVadParams* params, float crosstalk_db, int32_t* seg_start,
                                  int32_t* seg_end, int32_t* overlap, int32_t max_segments, int32_t* count, float* threshold_db, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---- language model: GPT-2 token negative log-likelihoods (lm.hip, lm_api.hip) --------------------------------------------------
 * The scorer of the reference's lms/ half: nll[b, s] = -log P(token s + 1 | tokens 0 .. s) under GPT-2 base (12 x 768 x 12 heads of 64
 * x 3072, checkpoint "gpt2"; any other width is refused by loco_lm_create with LOCO_E_INVALID naming the field -- gpt2-medium, -large
 * and -xl are out of scope).  Pre-LN blocks on the exact-fp32 GEMM (epilogue 5 = gelu_new for mlp.c_fc), the LayerNorm and the causal
 * wave-per-row attention the decoder uses (scale 1/8, key counts lens[b], no bias table), then ln_f and the tied LM head.
 *
 * Weights: loco_lm_set_weight takes HF's GPT2LMHeadModel names with or without the "transformer." prefix, fp32 on the device, and
 *   copies them (the handle owns its copies).  Conv1D weights come as HF stores them, [in, out]; loco_lm_finalize transposes them once.
 *   "*.attn.bias", "*.attn.masked_bias" and "lm_head.weight" are accepted and ignored: the head is tied to wte, of which there is one copy
 *   (a caller whose lm_head.weight differs from wte must refuse the checkpoint itself).  loco_lm_missing_weights returns the number of
 *   tensors still missing and writes their comma-separated names.
 * Sequences: `tokens` is ONE 1-D int32 device buffer -- a recording, or a corpus's utterances end to end; sequence b of a call is
 *   tokens[starts[b] .. starts[b] + lens[b]), starts / lens int32 [B] on the device, 0 <= lens[b] <= S <= n_positions <= 1024, position
 *   s of the model = offset s of the sequence.  Windows and ragged batches are thus formed on the device; rows beyond lens[b] embed as
 *   zeros and are never attended to.  The caller guarantees that starts[b] + lens[b] stays inside tokens.
 * Workspace: loco_lm_workspace_bytes(lm, B, S, R) bytes (R = 0 for loco_lm_forward), caller-owned; 0 for arguments outside the limits.
 *   Its first int32 is a status word: LOCO_LM_STATUS_CLEAN after a forward whose ids were all inside [0, vocab), else the smallest index
 *   into `tokens` of an id that was not (that token embedded as zeros); read it after the stream has completed the call.
 * loco_lm_nll: rows int32 [R] on the device are flat indices b * S + s of the positions to score; nll_out[r] scores position (b, s)
 *   against token s + 1 of sequence b, 0 where s + 1 >= lens[b], NaN for a row index outside [0, B S).  Only these R rows go through ln_f
 *   and the head, and the [R, vocab] logits are never formed: the head keeps a running (max, sum of exp, target logit) per row and
 *   vocabulary chunk of 1024 and merges a row's chunks in ascending order.  nll_out[r] is a function of that row's hidden state, its target
 *   and the weights alone, bit for bit: it does not depend on R or on r.
 * loco_lm_forward: for tests and small calls -- hidden_states (or NULL) are n_layer + 1 device pointers [B, S, 768] (each may be NULL):
 *   the embedding output, the residual stream after blocks 0 .. n_layer - 2, and ln_f of the last block's output, HF's
 *   output_hidden_states; logits (or NULL) [B, S, ldv] with ldv = loco_lm_vocab_stride (vocab rounded up to 4; columns >= vocab are 0),
 *   by the plain GEMM on wte.  B * S * ldv must stay below 2^31.
 * Operators (parity tests): loco_op_lm_head_nll is the head alone on h [R, 768] (already through ln_f) and targets int32 [R] (0 for
 *   ignore_index, NaN for another target outside [0, V)); V need not be a multiple of anything, columns >= V and rows >= R are never read;
 *   scratch >= loco_lm_head_scratch_bytes(R, V).  loco_op_lm_embed is the embedding (status: int32 [1] the caller set to
 *   LOCO_LM_STATUS_CLEAN, or NULL).  loco_op_lm_group_mean: mean[g] (double) of nll[offsets[g] .. offsets[g + 1]) summed in double in a
 *   fixed order, ppl[g] = exp(mean[g]); offsets int32 [G + 1] on the device.  loco_op_gemm's epilogue 5 is gelu_new. */
#define LOCO_LM_MAX_POSITIONS 1024
#define LOCO_LM_IGNORE_INDEX (-100)
#define LOCO_LM_STATUS_CLEAN 0x7f7f7f7f
typedef struct loco_lm loco_lm;
loco_lm* loco_lm_create(int32_t n_layer, int32_t n_positions, int32_t vocab, int32_t n_embd, int32_t n_head);
void loco_lm_destroy(loco_lm* lm);
int loco_lm_set_weight(loco_lm* lm, const char* hf_key, const void* dev_ptr, const int64_t* shape, int ndim);
int loco_lm_missing_weights(loco_lm* lm, char* names, size_t capacity);
int loco_lm_finalize(loco_lm* lm, void* stream);
int32_t loco_lm_vocab_stride(loco_lm* lm);
size_t loco_lm_workspace_bytes(loco_lm* lm, int32_t B, int32_t S, int32_t R);
int loco_lm_nll(loco_lm* lm, const int32_t* tokens, const int32_t* starts, const int32_t* lens, int32_t B, int32_t S, const int32_t* rows, int32_t R,
                float* nll_out, void* workspace, size_t workspace_bytes, void* stream);
int loco_lm_forward(loco_lm* lm, const int32_t* tokens, const int32_t* starts, const int32_t* lens, int32_t B, int32_t S, float* const* hidden_states,
                    float* logits, void* workspace, size_t workspace_bytes, void* stream);
size_t loco_lm_head_scratch_bytes(int64_t R, int32_t V);
int loco_op_lm_head_nll(const float* h, int64_t ldh, const float* wte, int64_t ldw, const int32_t* targets, int64_t R, int32_t V, int32_t ignore_index,
                        float* nll, void* scratch, size_t scratch_bytes, void* stream);
int loco_op_lm_embed(const int32_t* tokens, const int32_t* starts, const int32_t* lens, const float* wte, int32_t V, const float* wpe, float* x,
                     int32_t B, int32_t S, int32_t* status, void* stream);
int loco_op_lm_group_mean(const float* nll, const int32_t* offsets, int32_t G, double* mean, double* ppl, void* stream);

/* ---- language model with a cached context (lm_attention.hip, lm_api.hip) --------------------------------------------------------
 * A loco_lm_cache holds `slots` (1 .. 64) independent contexts: per slot and layer n_positions rows of k and of v in fp32, and the
 * residual row of the slot's last token, which predicts the token that follows the context.  A slot's length is host-side state
 * (loco_lm_cache_length: no synchronisation, -1 for a bad argument); it changes when a step is enqueued, so calls that share a cache must be
 * enqueued on one stream, by one thread at a time.  loco_lm_cache_reset sets a length to 0 and touches no device memory.
 *
 * loco_lm_ctx_step runs the model on N (1 .. 64) sequences of GPT-2 ids, each behind the tokens its slot already holds.  `tokens` is one
 * 1-D int32 device buffer, as for loco_lm_nll; `seqs` is a HOST array int32 [N][4] of (start, len, slot, flags): sequence n is
 * tokens[start .. start + len), stands at positions P .. P + len - 1 with P = the slot's length, and attends to the slot's P tokens and
 * causally to itself (csrc/lm_attention.hip).  flags:
 *   LOCO_LM_CTX_SCORE   nll_out receives len values, nll[t] = -log P(ids[t] | slot tokens, ids[:t]); token 0 is predicted from the slot's
 *                       stored last row and scores 0 on an empty slot.  The values of the scoring sequences are flat in sequence order.
 *   LOCO_LM_CTX_COMMIT  the sequence's k / v rows of every layer are appended to the slot, its last row replaces the slot's, and the length
 *                       grows by len.  At most one committing sequence per slot and call.
 * Any number of sequences may read one slot (an n-best list); a slot changes only through a commit, and every sequence of a call sees
 * the slots as they were before the call.  Refused by name before any launch: P + len > n_positions, len < 1, a slot out of range, two
 * commits on one slot, a null argument, a workspace below loco_lm_ctx_workspace_bytes(lm, rows, N) (rows = the sum of len; 0 outside the
 * limits).  The call allocates nothing, never synchronises and runs on the caller's stream; the workspace's first int32 is the status
 * word of loco_lm_nll.
 * Bits: a sequence's values are a function of its ids, its slot's contents and P alone -- not of N, of the sequences beside it or of the
 * slot's index.  A context built in several commits and the same tokens committed at once partition the keys differently and agree to
 * fp32 rounding, not to the bit; for a given chunking the result is bit-reproducible.
 * loco_op_lm_ctx_attention is the attention kernel alone: qkv packed rows of q | k | v (row stride 2304), kcache / vcache
 * [slots][rows][768] with slot_stride floats between slots, seqs a HOST array int32 [N][3] of (len, slot, P), out packed rows of 768. */
#define LOCO_LM_CTX_SCORE 1
#define LOCO_LM_CTX_COMMIT 2
#define LOCO_LM_CTX_MAX_SEQS 64
#define LOCO_LM_CACHE_MAX_SLOTS 64
typedef struct loco_lm_cache loco_lm_cache;
loco_lm_cache* loco_lm_cache_create(loco_lm* lm, int32_t slots);
void loco_lm_cache_destroy(loco_lm_cache* cache);
int loco_lm_cache_reset(loco_lm_cache* cache, int32_t slot);
int32_t loco_lm_cache_length(loco_lm_cache* cache, int32_t slot);
size_t loco_lm_ctx_workspace_bytes(loco_lm* lm, int32_t rows, int32_t N);
int loco_lm_ctx_step(loco_lm* lm, loco_lm_cache* cache, const int32_t* tokens, const int32_t* seqs, int32_t N, float* nll_out, void* workspace,
                     size_t workspace_bytes, void* stream);
int loco_op_lm_ctx_attention(const float* qkv, const float* kcache, const float* vcache, int64_t slot_stride, const int32_t* seqs, int32_t N,
                             int32_t slots, float* out, void* stream);

/* ---- error rates: edit distance over symbol sequences, n-best risk (edit_distance.hip) ------------------------------------------
 * The rule is integer and exact.  For a reference a[0..n) and a hypothesis b[0..m) of int32 symbols a cell is the pair (cost, S),
 * compared lexicographically:
 *     D[i][0] = (i, 0)        D[0][j] = (j, 0)
 *     D[i][j] = min( D[i-1][j-1] + (a[i-1] == b[j-1] ? (0,0) : (1,1)),    hit / substitution
 *                    D[i-1][j]   + (1,0),                                  deletion
 *                    D[i][j-1]   + (1,0) )                                 insertion
 * and the result is (cost, S) = D[n][m]: the minimum edit distance and, among the alignments of that cost, the fewest substitutions.
 * D - I = n - m and D + I = cost - S give D and I; hits = n - S - D.  For a fixed cost the fewest substitutions is the most hits:
 * MINIMUM COST, THEN MOST CORRECT SYMBOLS.  Swapping the two sides keeps cost and S and swaps D with I.  The result is a property of
 * the pair, not of a traceback order.  It is this library's own tie rule: cost, and so every error RATE, is what sclite and Kaldi
 * compute, while the split into S / D / I can differ from theirs where alignments tie.
 *
 * loco_op_edit_distance: `symbols` int32 [n_symbols] and `spans` int32 [P][4] = ref_start, ref_len, hyp_start, hyp_len on the device
 * (spans may overlap or coincide); counts int32 [P][4] = S, D, I, hits.  A side holds at most loco_edit_max_len() = LOCO_EDIT_MAX_LEN
 * symbols.  `max_len` (0 .. LOCO_EDIT_MAX_LEN) is the longest min(ref_len, hyp_len) the caller expects among the pairs: it sizes the
 * row state a wave keeps in LDS (LOCO_EDIT_MAX_LEN always serves; a close bound is faster).  A pair gets counts = -1, -1, -1, -1, and
 * nothing of it is read, when a length is negative or above the cap, a span leaves [0, n_symbols), or min(ref_len, hyp_len) > max_len.
 * ref_len = 0 or hyp_len = 0 is legal (all insertions / all deletions).  A pair's four numbers depend on its own two spans alone --
 * not on P, on its place in the launch, on max_len or on its neighbours.
 * loco_op_nbest_risk: group u holds the hypotheses group_offsets[u] .. group_offsets[u + 1] (int32 [U + 1], ascending); `counts` is
 * loco_op_edit_distance's output for every group's N (N - 1) / 2 pairs (i < j) in row-major order, group after group.
 *     risk[h] = (sum over h' != h of w[h'] * cost(h, h')) / (sum over h' of w[h']),   cost = S + D + I,
 * in double, h' ascending, every product and every sum rounded on its own (no fused multiply-add); `weights` double [total] or NULL
 * = all 1 (Monte-Carlo MBR over samples of the model).  best[u] = the first index within the group of least risk; one hypothesis
 * gives risk 0 and best 0, an empty group best -1.  risk double [total], best int32 [U].
 * LOCO_E_INVALID before any device work: a null pointer (weights excepted), P < 0, U < 0, n_symbols outside 0 .. 2^31 - 1, max_len
 * outside 0 .. LOCO_EDIT_MAX_LEN, symbols / counts / group_offsets / best not 4-byte aligned, spans not 16-byte aligned, weights /
 * risk not 8-byte aligned.  P = 0 and U = 0 do nothing.  No allocation, no synchronisation; the caller's stream. */
#define LOCO_EDIT_MAX_LEN 16384
int32_t loco_edit_max_len(void);
int loco_op_edit_distance(const int32_t* symbols, int64_t n_symbols, const int32_t* spans, int32_t P, int32_t max_len, int32_t* counts,
                          void* stream);
int loco_op_nbest_risk(const int32_t* counts, const int32_t* group_offsets, const double* weights, int32_t U, double* risk, int32_t* best,
                       void* stream);

/* ---- embedding neighbours: row norms, fused top-k, group mean (neighbors.hip) ---------------------------------------------------
 * Which rows of K [N, 768] are closest to each row of Q [M, 768], without an M x N matrix: the exact-fp32 MFMA product is walked in
 * 128 x 128 tiles and every query keeps a sorted list of its k best keys.  All pointers are device pointers; dim must be 768.
 *
 * loco_op_row_norm2: norm2[r] = the squared norm of x's row r (row stride ldx floats), summed in double in one written order (lane l
 * of a wave sums elements l, l + 64, ... ascending, then a butterfly) and rounded to fp32 once.
 *
 * loco_op_topk: values f32 [M][k] and indices i32 [M][k], best first, ties towards the LOWER key index.  Q and K are fp32 with row
 * strides ldq / ldk (multiples of 4, >= 768, ldq < 2^23; both bases 16-byte aligned).  Metrics, s = the score, larger is better:
 *     LOCO_TOPK_DOT      s = q.k
 *     LOCO_TOPK_COSINE   s = ((q.k) * inv_q) * inv_k,  inv = 1 / max(sqrt(norm2), 1e-12)   (torch.nn.functional.normalize's eps; a zero
 *                        vector scores 0)
 *     LOCO_TOPK_L2       s = (2 (q.k) - norm2_k) - norm2_q   (the negated squared distance)
 * q_norm2 [M] and k_norm2 [N] are loco_op_row_norm2's outputs (ignored, and may be NULL, for DOT).  exclude i32 [M] (or NULL) names
 * one key index per query that is not a candidate, -1 for none (leave-one-out, self-similarity).  A NaN score is not a candidate.
 * Where fewer than k candidates exist the remaining slots hold index -1 and value -inf.  k is 1 .. loco_topk_max_k() =
 * LOCO_TOPK_MAX_K.  scratch holds one record of k pairs per (query, chunk of 1024 keys): loco_topk_scratch_bytes(M, N, k) =
 * 8 M ceil(N / 1024) k bytes (0 outside the limits), 16-byte aligned; a caller bounds it by splitting M, which changes no result.
 * Bits: a query's k results are a function of that query's 768 values, its norm, its exclude entry and the keys alone -- not of M, of
 * the query's row, of the split of M or of the queries beside it: a score is one MFMA chain in the tile walk's k order, tiles and
 * chunks start at multiples of 128 from key 0, and the chunk records are merged in ascending order by (value desc, index asc).
 * Keys >= N and queries >= M are never read.
 *
 * loco_op_group_mean: out[g][:] = the mean of rows[index[j]][:] over j in [offsets[g], offsets[g + 1]) (offsets int64 [G + 1],
 * ascending; index int32, or NULL for the contiguous run rows[j]).  Sums are in double in an order that depends on the group's size
 * alone (row j goes to partial sum j mod 4 ascending; the four are added in order), divided and rounded to fp32 once.  count i32 [G]
 * (or NULL) gets the group sizes.  An EMPTY group leaves out[g] untouched and sets count[g] = 0.  A row index outside [0, n_rows) is
 * not read and makes its group's mean NaN.  It serves mean pooling of a ragged store and the k-means centre update (index = points
 * stably sorted by label).  No floating-point atomics anywhere.
 * LOCO_E_INVALID before any device work, naming the argument: a null pointer (the nullable ones excepted), dim != 768, k or metric out
 * of range, M / N / G / rows outside 1 .. 2^31 - 1, a stride or an alignment as above; LOCO_E_WORKSPACE for a short scratch.  No
 * allocation, no synchronisation; the caller's stream. */
#define LOCO_TOPK_MAX_K 16
#define LOCO_TOPK_DOT 0
#define LOCO_TOPK_COSINE 1
#define LOCO_TOPK_L2 2
int32_t loco_topk_max_k(void);
size_t loco_topk_scratch_bytes(int64_t M, int64_t N, int32_t k);
int loco_op_row_norm2(const float* x, int64_t ldx, int64_t rows, int32_t dim, float* norm2, void* stream);
int loco_op_topk(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* q_norm2, const float* k_norm2, const int32_t* exclude,
                 int64_t M, int64_t N, int32_t dim, int32_t k, int32_t metric, float* values, int32_t* indices, void* scratch,
                 size_t scratch_bytes, void* stream);
int loco_op_group_mean(const float* rows, int64_t ld, int64_t n_rows, const int32_t* index, const int64_t* offsets, int64_t G, int32_t dim,
                       float* out, int64_t ldo, int32_t* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LOCO_ASR_H */
